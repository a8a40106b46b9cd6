// hsr_keyframe_pack.hip — a keyframe's float32 colour, float32 depth and int64 label planes as 8-/16-bit codes and back (gfx950),
// DESIGN.md §7 row 13.  See include/ext/hsr_keyframe_pack.h for the three rules, step by step.
//   pack_kernel<V>   : blockIdx.y is the plane (0..2 colour, 3 depth, 4.. labels), blockIdx.x a run of 1024 values of it.  V = 4: a lane
//                      takes 4 consecutive values of the plane's flat index: one 16-byte load per float plane (two per int64 plane), one
//                      4-byte store of 4 colour codes or one 8-byte store of 4 16-bit codes; the last N % 4 values of the plane go one
//                      at a time.  V = 1: a lane takes 4 values 256 apart, one at a time, for calls with a base pointer off its vector
//                      alignment.  Every workgroup leaves the number of its values that the codes do not reproduce in partials[plane][x].
//   finish_kernel    : one workgroup adds the partials of each group into lossy[3] (64-bit sums, stored saturated).
//   unpack_kernel<V> : the same indexing, the other way.
// A plane of N % 4 != 0 values puts the next plane off the vector's natural alignment: the vector accesses are declared with the
// element's alignment (4 for float, 8 for int64, 1 for the colour codes, 2 for the 16-bit codes) and the compiler picks an access
// global memory takes at that alignment (hsr_lane_io.h: the vector types, hsr_load<V> and hsr_store<V>).  Streaming, bound by bytes:
// a 1200x680 keyframe with 5 label planes reads 45.7 MB and writes 12.2 MB; nothing is reused across lanes, so nothing is staged in
// LDS.  Compiled with -ffp-contract=off: the rules have one product each and no sum next to it; the flag keeps them as written.
#include <math.h>

#include "hsr_common.h"
#include "hsr_block.h"
#include "hsr_lane_io.h"
#include "hsr_ingest_expr.h"
#include "../../include/hsr_eval.h"
#include "../../include/ext/hsr_frame_resample.h"
#include "../../include/ext/hsr_keyframe_pack.h"

static_assert(HSR_KEYFRAME_MAX_SIDE == HSR_RESAMPLE_MAX_SIDE, "a keyframe is as large as an ingested frame");
static_assert(HSR_KEYFRAME_MAX_PLANES == HSR_EVAL_MAX_LEVELS + 1, "the tree levels and the leaf plane");

namespace {

constexpr int PB = 256;
constexpr int PER_BLOCK = 4 * PB;      // values of one plane per workgroup, in both paths
constexpr int COLOUR_PLANES = 3, DEPTH_PLANE = 3, FIRST_LABEL_PLANE = 4;

struct PackArgs {
    long long N;
    const float* color;
    const float* depth;
    const long long* labels;
    double depth_scale;
    uint8_t* out_color;
    uint16_t* out_depth;
    uint16_t* out_labels;
    unsigned* partials;      // [4 + L][gridDim.x]
};

struct UnpackArgs {
    long long N;
    const uint8_t* color;
    const uint16_t* depth;
    const uint16_t* labels;
    double depth_scale;
    float* out_color;
    float* out_depth;
    long long* out_labels;
};

// ---- the three rules on one value: the code, and whether it reproduces the value ----
__device__ __forceinline__ unsigned colour_code(float c, unsigned& bad)
{
    float t = c * 255.0f;
    t = t > 0.f ? (t < 255.f ? t : 255.f) : 0.f;      // a NaN fails t > 0
    const float v = rintf(t);                          // to nearest, halves to even
    bad += __float_as_uint(hsr_ingest_colour(v)) != __float_as_uint(c) ? 1u : 0u;
    return (unsigned)v;
}

__device__ __forceinline__ unsigned depth_code(float d, double scale, unsigned& bad)
{
    double t = (double)d * scale;
    t = t > 0.0 ? (t < 65535.0 ? t : 65535.0) : 0.0;  // a NaN fails t > 0
    const double q = rint(t);
    bad += __float_as_uint(hsr_ingest_depth(q, scale)) != __float_as_uint(d) ? 1u : 0u;
    return (unsigned)q;
}

__device__ __forceinline__ unsigned label_code(long long l, unsigned& bad)
{
    bad += (l < 0 || l > 65535) ? 1u : 0u;
    return (unsigned)(l < 0 ? 0 : (l > 65535 ? 65535 : l));
}

// `plane` is uniform over the workgroup; at = plane * N + i, the flat index into the group's first plane
template <int V>
__device__ __forceinline__ void pack_values(const PackArgs& a, int plane, size_t i, unsigned& bad)
{
    unsigned code[V];
    if (plane < COLOUR_PLANES) {
        const size_t at = (size_t)plane * (size_t)a.N + i;
        float c[V];
        hsr_load<V>(a.color + at, c);
#pragma unroll
        for (int v = 0; v < V; v++) code[v] = colour_code(c[v], bad);
        hsr_store<V>(a.out_color + at, code);
    } else if (plane == DEPTH_PLANE) {
        float d[V];
        hsr_load<V>(a.depth + i, d);
#pragma unroll
        for (int v = 0; v < V; v++) code[v] = depth_code(d[v], a.depth_scale, bad);
        hsr_store<V>(a.out_depth + i, code);
    } else {
        const size_t at = (size_t)(plane - FIRST_LABEL_PLANE) * (size_t)a.N + i;
        long long l[V];
        hsr_load<V>(a.labels + at, l);
#pragma unroll
        for (int v = 0; v < V; v++) code[v] = label_code(l[v], bad);
        hsr_store<V>(a.out_labels + at, code);
    }
}

template <int V>
__device__ __forceinline__ void unpack_values(const UnpackArgs& a, int plane, size_t i)
{
    unsigned code[V];
    float x[V];
    if (plane < COLOUR_PLANES) {
        const size_t at = (size_t)plane * (size_t)a.N + i;
        hsr_load<V>(a.color + at, code);
#pragma unroll
        for (int v = 0; v < V; v++) x[v] = hsr_ingest_colour((float)code[v]);
        hsr_store<V>(a.out_color + at, x);
    } else if (plane == DEPTH_PLANE) {
        hsr_load<V>(a.depth + i, code);
#pragma unroll
        for (int v = 0; v < V; v++) x[v] = hsr_ingest_depth((double)code[v], a.depth_scale);
        hsr_store<V>(a.out_depth + i, x);
    } else {
        const size_t at = (size_t)(plane - FIRST_LABEL_PLANE) * (size_t)a.N + i;
        hsr_load<V>(a.labels + at, code);
        hsr_store<V>(a.out_labels + at, code);
    }
}

// is plane `plane` of the call present?  (an absent group's workgroups do nothing; the pack's still write their zero count)
template <typename Args>
__device__ __forceinline__ bool present(const Args& a, int plane)
{
    return plane < COLOUR_PLANES ? a.color != nullptr : (plane == DEPTH_PLANE ? a.depth != nullptr : true);
}

template <int V>
__global__ __launch_bounds__(PB) void pack_kernel(PackArgs a)
{
    __shared__ unsigned s_red[PB / 64];
    const int plane = blockIdx.y;
    const long long base = (long long)blockIdx.x * PER_BLOCK;      // < N <= 2^28
    unsigned bad = 0;
    if (present(a, plane)) {
        if (V == 4) {
            const long long i = base + (long long)threadIdx.x * 4;
            if (i + 4 <= a.N) {
                pack_values<4>(a, plane, (size_t)i, bad);
            } else {
                for (long long k = i; k < a.N; k++) pack_values<1>(a, plane, (size_t)k, bad);      // the last N % 4 values
            }
        } else {
#pragma unroll
            for (int it = 0; it < 4; it++) {
                const long long i = base + it * PB + threadIdx.x;
                if (i < a.N) pack_values<1>(a, plane, (size_t)i, bad);
            }
        }
    }
    const unsigned total = hsr_block256_isum(bad, s_red);      // <= 1024
    if (threadIdx.x == 0) a.partials[(size_t)plane * gridDim.x + blockIdx.x] = total;
}

// lossy[g] = the sum of the partials of group g's planes: colour [0, 3 nbx), depth [3 nbx, 4 nbx), labels [4 nbx, (4 + L) nbx)
__global__ __launch_bounds__(PB) void finish_kernel(const unsigned* __restrict__ partials, unsigned nbx, int L, unsigned* __restrict__ lossy)
{
    __shared__ unsigned long long s_red[PB / 64][3], s_sum[3];
    const size_t end[4] = {0, (size_t)COLOUR_PLANES * nbx, (size_t)FIRST_LABEL_PLANE * nbx, (size_t)(FIRST_LABEL_PLANE + L) * nbx};
    unsigned long long c[3] = {0ull, 0ull, 0ull};
    // eight loads in flight per thread: one workgroup reads every partial, and a load at a time is a latency per load
#pragma unroll
    for (int g = 0; g < 3; g++)
        for (size_t k = end[g] + threadIdx.x; k < end[g + 1]; k += 8 * PB) {
            unsigned v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const size_t at = k + (size_t)u * PB;
                v[u] = at < end[g + 1] ? partials[at] : 0u;      // each <= 1024
            }
            c[g] += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
        }
    hsr_block256_sums(c, s_red, s_sum);      // thread g < 3 writes s_sum[g], and reads its own word back
    if (threadIdx.x < 3) lossy[threadIdx.x] = s_sum[threadIdx.x] > 0xffffffffull ? 0xffffffffu : (unsigned)s_sum[threadIdx.x];
}

template <int V>
__global__ __launch_bounds__(PB) void unpack_kernel(UnpackArgs a)
{
    const int plane = blockIdx.y;
    if (!present(a, plane)) return;
    const long long base = (long long)blockIdx.x * PER_BLOCK;
    if (V == 4) {
        const long long i = base + (long long)threadIdx.x * 4;
        if (i + 4 <= a.N) {
            unpack_values<4>(a, plane, (size_t)i);
        } else {
            for (long long k = i; k < a.N; k++) unpack_values<1>(a, plane, (size_t)k);
        }
    } else {
#pragma unroll
        for (int it = 0; it < 4; it++) {
            const long long i = base + it * PB + threadIdx.x;
            if (i < a.N) unpack_values<1>(a, plane, (size_t)i);
        }
    }
}

unsigned blocks_x(int H, int W) { return (unsigned)(((size_t)H * W + PER_BLOCK - 1) / PER_BLOCK); }      // <= 2^18

// the checks both entries share; `wide`: the float / int64 side, `codes`: the 8-/16-bit side of each group
int check(const char* who, int H, int W, int L, double depth_scale, const void* wide_color, const void* code_color, const void* wide_depth,
          const void* code_depth, const void* wide_labels, const void* code_labels, bool packing)
{
    if (H < 1 || H > HSR_KEYFRAME_MAX_SIDE || W < 1 || W > HSR_KEYFRAME_MAX_SIDE) {
        hsr_set_error("%s: sides must be 1..%d; got %dx%d", who, HSR_KEYFRAME_MAX_SIDE, H, W);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (L < 0 || L > HSR_KEYFRAME_MAX_PLANES) {
        hsr_set_error("%s: L must be 0..%d; got %d", who, HSR_KEYFRAME_MAX_PLANES, L);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!isfinite(depth_scale) || depth_scale == 0.0) {
        hsr_set_error("%s: depth_scale must be finite and non-zero; got %g", who, depth_scale);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const void* in_color = packing ? wide_color : code_color;
    const void* in_depth = packing ? wide_depth : code_depth;
    const void* out_color = packing ? code_color : wide_color;
    const void* out_depth = packing ? code_depth : wide_depth;
    if ((in_color && !out_color) || (in_depth && !out_depth)) {
        hsr_set_error("%s: colour or depth given without its output", who);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (L > 0 ? (!wide_labels || !code_labels) : (wide_labels || code_labels)) {
        hsr_set_error("%s: labels given without an output (or the reverse), or not as L says: L=%d takes %s", who, L,
                      L > 0 ? "both pointers" : "both NULL");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!in_color && !in_depth && L == 0) {
        hsr_set_error("%s: nothing to do: colour and depth are NULL and L is 0", who);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    return HSR_OK;
}

// may every group's base pointer take the 4-value accesses?  (float and int64 planes 16 bytes, colour codes 4, 16-bit codes 8)
bool vector_path(const void* wide_color, const void* code_color, const void* wide_depth, const void* code_depth, const void* wide_labels,
                 const void* code_labels)
{
    return hsr_aligned(wide_color, 16) && hsr_aligned(wide_depth, 16) && hsr_aligned(wide_labels, 16) && hsr_aligned(code_color, 4) &&
           hsr_aligned(code_depth, 8) && hsr_aligned(code_labels, 8);
}

}  // namespace

extern "C" size_t hsr_keyframe_pack_scratch_bytes(int H, int W, int L)
{
    if (H < 1 || H > HSR_KEYFRAME_MAX_SIDE || W < 1 || W > HSR_KEYFRAME_MAX_SIDE || L < 0 || L > HSR_KEYFRAME_MAX_PLANES) return 1024;
    return hsr_align256((size_t)(FIRST_LABEL_PLANE + L) * blocks_x(H, W) * sizeof(unsigned));
}

extern "C" int hsr_keyframe_pack(int H, int W, const float* color, const float* depth, int L, const int64_t* labels, double depth_scale,
                                 uint8_t* out_color, uint16_t* out_depth, uint16_t* out_labels, uint32_t* lossy, char* scratch,
                                 size_t scratch_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = check("keyframe_pack", H, W, L, depth_scale, color, out_color, depth, out_depth, labels, out_labels, true);
    if (rc != HSR_OK) return rc;
    if (!lossy) {
        hsr_set_error("keyframe_pack: NULL lossy");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const size_t need = hsr_keyframe_pack_scratch_bytes(H, W, L);
    if (!scratch || scratch_bytes < need || !hsr_aligned(scratch, 4)) {
        hsr_set_error("keyframe_pack: scratch too small: %zu bytes needed, %zu given (or NULL, or not 4-byte aligned)", need, scratch_bytes);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const unsigned nbx = blocks_x(H, W);
    unsigned* partials = reinterpret_cast<unsigned*>(scratch);
    const PackArgs a{(long long)H * W, color, depth, reinterpret_cast<const long long*>(labels), depth_scale, out_color, out_depth, out_labels,
                     partials};
    const dim3 grid(nbx, FIRST_LABEL_PLANE + L);
    if (vector_path(color, out_color, depth, out_depth, labels, out_labels))
        pack_kernel<4><<<grid, PB, 0, stream>>>(a);
    else
        pack_kernel<1><<<grid, PB, 0, stream>>>(a);
    finish_kernel<<<1, PB, 0, stream>>>(partials, nbx, L, lossy);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_keyframe_unpack(int H, int W, const uint8_t* color_u8, const uint16_t* depth_u16, int L, const uint16_t* labels_u16,
                                   double depth_scale, float* out_color, float* out_depth, int64_t* out_labels, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = check("keyframe_unpack", H, W, L, depth_scale, out_color, color_u8, out_depth, depth_u16, out_labels, labels_u16, false);
    if (rc != HSR_OK) return rc;
    const UnpackArgs a{(long long)H * W, color_u8, depth_u16, labels_u16, depth_scale, out_color, out_depth,
                       reinterpret_cast<long long*>(out_labels)};
    const dim3 grid(blocks_x(H, W), FIRST_LABEL_PLANE + L);
    if (vector_path(out_color, color_u8, out_depth, depth_u16, out_labels, labels_u16))
        unpack_kernel<4><<<grid, PB, 0, stream>>>(a);
    else
        unpack_kernel<1><<<grid, PB, 0, stream>>>(a);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}
