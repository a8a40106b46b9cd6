// hsr_replay.hip — the replay of a finished run (gfx950): the map as it stood at step t, and a rendered view as a coloured world-space
// point cloud (include/ext/hsr_replay.h, which states every rule and the reference lines, viz_scripts/online_recon_sem_replica.py).
//   plan   : plan_hist_kernel — the step each row first shows at, one integer atomic per run of equal steps within a wave (rows arrive in
//            long runs: the first frame alone is often a third of the map); plan_scan_kernel — one workgroup, hsr_block.h's exclusive
//            scan of the T bins, turned inclusive.
//   select : select_count_kernel / select_scan_kernel / select_emit_kernel, the count / scan / emit of hsr_densify.hip.  The emit runs
//            hsr_view_row.h's row function (hsr_view_prep's own: 36-44 B read and 44-60 B written per selected row, float4 for the [P,4]
//            rows) with the rank as the destination row, copies the colour row, and copies the K semantic columns FLAT: the block leaves
//            its 256 destination rows in LDS and walks its 256 * K source floats with the lanes along the flat index, so reads are
//            coalesced and writes are wherever neighbours are both selected (a row per lane would stride the lanes by 4 K bytes).
//   cloud  : cloud_kernel<V> — hsr_block.h's back-projection per pixel; V = 4: a lane owns four pixels, 60 record bytes = 15 aligned
//            dwords and 12 floats of points (hsr_lane_io.h's vector types); V = 1 for the tail and for records off a dword.
// Compiled with -ffp-contract=off: the select's outputs must equal hsr_view_prep's bit for bit and the cloud's chain is pinned against
// a float32 restatement that rounds every operation once.
#include <math.h>

#include "hsr_common.h"
#include "hsr_block.h"
#include "hsr_lane_io.h"
#include "hsr_view_row.h"
#include "../../include/ext/hsr_replay.h"

namespace {

constexpr int RB = 256;
constexpr int MAX_P = 0x7fffff00;      // the last block's row indices stay below 2^31

// ---- plan ------------------------------------------------------------------------------------------------------------------------------
// the step row p first shows at, the smallest integer t >= ts; -1: never (NaN, +inf, above T - 1).  Compared in float first: (int) of
// a large float is undefined
__device__ __forceinline__ int first_step(float ts, int T)
{
    if (!(ts <= (float)(T - 1))) return -1;
    return ts <= 0.f ? 0 : (int)ceilf(ts);
}

__global__ __launch_bounds__(RB) void plan_hist_kernel(int P, int T, const float* __restrict__ timestep, unsigned* __restrict__ hist)
{
    const int p = blockIdx.x * RB + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int bin = p < P ? first_step(timestep[p], T) : -1;
    const int below = __shfl_up(bin, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || bin != below);      // bit l: a run of equal bins starts at lane l
    if (!((heads >> lane) & 1ull) || bin < 0) return;
    const unsigned long long later = lane == 63 ? 0ull : heads >> (lane + 1);
    const int len = later ? __ffsll((long long)later) : 64 - lane;            // lanes up to the next head, or to the end of the wave
    atomicAdd(&hist[bin], (unsigned)len);                                        // integers: any order gives the same counts
}

__global__ __launch_bounds__(1024) void plan_scan_kernel(int T, unsigned* __restrict__ hist, long long* __restrict__ out_upto)
{
    __shared__ unsigned s_w[17];
    // inclusive = count + exclusive prefix, each thread on the bins the scan gives it (hsr_block.h): no thread reads another's
    const int per = (T + 1023) / 1024, beg = threadIdx.x * per;
    for (int t = beg; t < beg + per && t < T; t++) out_upto[t] = (long long)hist[t];
    hsr_block1024_exclusive_scan(T, hist, s_w);
    for (int t = beg; t < beg + per && t < T; t++) out_upto[t] += (long long)hist[t];
}

// ---- select ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool shown(const float* __restrict__ timestep, int p, int P, float step) { return p < P && timestep[p] <= step; }

__global__ __launch_bounds__(RB) void select_count_kernel(int P, float step, const float* __restrict__ timestep, unsigned* __restrict__ counts)
{
    __shared__ unsigned s_w[4];
    const unsigned n = hsr_block256_count(shown(timestep, blockIdx.x * RB + threadIdx.x, P, step), s_w);
    if (threadIdx.x == 0) counts[blockIdx.x] = n;
}

__global__ __launch_bounds__(1024) void select_scan_kernel(int nblk, unsigned* __restrict__ counts, int* __restrict__ out_count)
{
    __shared__ unsigned s_w[17];
    const unsigned total = hsr_block1024_exclusive_scan(nblk, counts, s_w);
    if (threadIdx.x == 0) *out_count = (int)total;
}

struct SelectOut {
    float *means3D, *unnorm_rot, *rotations, *opacities, *scales, *colors, *semantic;
    int* index;
};

template <bool WORLD>
__global__ __launch_bounds__(RB) void select_emit_kernel(ViewArgs a, int K, float step, unsigned capacity, const float* __restrict__ timestep,
                                                         const float* __restrict__ rgb_colors, const float* __restrict__ semantic,
                                                         const unsigned* __restrict__ offsets, SelectOut o)
{
    __shared__ unsigned s_w[4];
    __shared__ unsigned s_dst[RB];      // the destination row of each of the block's rows, or NO_ROW
    constexpr unsigned NO_ROW = 0xffffffffu;
    const int base = blockIdx.x * RB;
    const int p = base + threadIdx.x;
    const bool m = shown(timestep, p, a.P, step);
    const unsigned rank = hsr_block_rank<4>(m, s_w);   // holds the barrier: no thread returns before it
    const unsigned pos = offsets[blockIdx.x] + rank;
    const bool write = m && pos < capacity;
    if (write) {
        view_row<WORLD>(a, (size_t)p, (size_t)pos, o.means3D, o.unnorm_rot, o.rotations, o.opacities, o.scales);
#pragma unroll
        for (int c = 0; c < 3; c++) o.colors[3 * (size_t)pos + c] = rgb_colors[3 * (size_t)p + c];
        if (o.index) o.index[pos] = p;
    }
    if (K == 0 || !o.semantic) return;      // uniform over the launch
    s_dst[threadIdx.x] = write ? pos : NO_ROW;
    __syncthreads();
    const int rows = min(RB, a.P - base);
    const int flat = rows * K;                // <= 256 * K: K < 2^23 is checked on the host
    const int dq = RB / K, dr = RB - dq * K;  // one trip moves the flat index by 256 = dq rows and dr columns
    int row = threadIdx.x / K, col = threadIdx.x - row * K;
    const float* __restrict__ src = semantic + (size_t)base * K;
    for (int f = threadIdx.x; f < flat; f += RB) {
        const unsigned d = s_dst[row];
        if (d != NO_ROW) o.semantic[(size_t)d * K + col] = src[f];
        row += dq;
        col += dr;
        if (col >= K) { col -= K; row++; }
    }
}

// ---- cloud -----------------------------------------------------------------------------------------------------------------------------
// `bytes` bytes of v (little-endian) at byte offset `at` of the packed dwords w (zero before the first call): constant offsets after unrolling
template <int WORDS>
__device__ __forceinline__ void put(unsigned (&w)[WORDS], int at, unsigned v, int bytes)
{
    const int k = at >> 2, sh = (at & 3) * 8;
    w[k] |= v << sh;
    if (sh + 8 * bytes > 32) w[k + 1] |= v >> (32 - sh);
}

// V pixels from flat index i on (V = 4: i is a multiple of 4 and out_records 4-byte aligned)
template <int V>
__device__ __forceinline__ void cloud_pixels(size_t i, int W, const float* __restrict__ depth, const uint8_t* __restrict__ picture,
                                             const hsr_pinhole& f, const float* __restrict__ c2w, float* __restrict__ out_points,
                                             uint8_t* __restrict__ out_records)
{
    float pts[V][3];
#pragma unroll
    for (int v = 0; v < V; v++) {
        const size_t n = i + v;      // < 2^31
        const int py = (int)((unsigned)n / (unsigned)W), px = (int)((unsigned)n - (unsigned)py * (unsigned)W);
        hsr_backproject((float)px, (float)py, depth[n], f, c2w, pts[v]);
    }
    if (out_points) {
        float* __restrict__ op = out_points + 3 * i;
        if (V == 4) {
#pragma unroll
            for (int q = 0; q < 3; q++) {
                hsr_f4 t;
                t.x = pts[(4 * q) / 3][(4 * q) % 3]; t.y = pts[(4 * q + 1) / 3][(4 * q + 1) % 3];
                t.z = pts[(4 * q + 2) / 3][(4 * q + 2) % 3]; t.w = pts[(4 * q + 3) / 3][(4 * q + 3) % 3];
                reinterpret_cast<hsr_f4_a4*>(op)[q] = t;
            }
        } else {
            op[0] = pts[0][0]; op[1] = pts[0][1]; op[2] = pts[0][2];
        }
    }
    if (!out_records) return;
    const uint8_t* __restrict__ pic = picture + 3 * i;
    uint8_t* __restrict__ rec = out_records + 15 * i;
    if (V == 4) {
        unsigned w[15];
#pragma unroll
        for (int k = 0; k < 15; k++) w[k] = 0u;
#pragma unroll
        for (int v = 0; v < 4; v++) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                put(w, 15 * v + 4 * c, __float_as_uint(pts[v][c]), 4);
                put(w, 15 * v + 12 + c, (unsigned)pic[3 * v + c], 1);
            }
        }
        unsigned* __restrict__ ow = reinterpret_cast<unsigned*>(rec);
#pragma unroll
        for (int k = 0; k < 15; k++) ow[k] = w[k];
    } else {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const unsigned b = __float_as_uint(pts[0][c]);
            rec[4 * c] = (uint8_t)b; rec[4 * c + 1] = (uint8_t)(b >> 8); rec[4 * c + 2] = (uint8_t)(b >> 16); rec[4 * c + 3] = (uint8_t)(b >> 24);
            rec[12 + c] = pic[c];
        }
    }
}

template <int V>
__global__ __launch_bounds__(RB) void cloud_kernel(long long N, int W, const float* __restrict__ depth, const uint8_t* __restrict__ picture,
                                                   hsr_pinhole f, const float* __restrict__ c2w, float* __restrict__ out_points,
                                                   uint8_t* __restrict__ out_records)
{
    const long long i = ((long long)blockIdx.x * RB + threadIdx.x) * V;
    if (i + V <= N) {
        cloud_pixels<V>((size_t)i, W, depth, picture, f, c2w, out_points, out_records);
    } else if (V > 1) {
        for (long long k = i; k < N; k++) cloud_pixels<1>((size_t)k, W, depth, picture, f, c2w, out_points, out_records);   // the last H * W % 4
    }
}

size_t select_blocks(int P) { return ((size_t)(P > 0 ? P : 1) + RB - 1) / RB; }

// the replay's own scratch check: a refusal like the rest (HSR_ERR_INVALID_ARGUMENT), not hsr_check_scratch's BUFFER_TOO_SMALL
bool bad_scratch(const char* who, const char* scratch, size_t have, size_t need)
{
    if (scratch && have >= need && hsr_aligned(scratch, 4)) return false;
    hsr_set_error("%s: scratch too small: %zu bytes needed, %zu given (or NULL, or not 4-byte aligned)", who, need, have);
    return true;
}

}  // namespace

extern "C" size_t hsr_replay_plan_scratch_bytes(int P, int T)
{
    (void)P;
    if (T < 1 || T > HSR_REPLAY_MAX_STEPS) return 256;
    return hsr_align256((size_t)T * sizeof(unsigned));
}

extern "C" int hsr_replay_plan(int P, int T, const float* timestep, int64_t* out_upto, char* scratch, size_t scratch_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || P > MAX_P || T < 1 || T > HSR_REPLAY_MAX_STEPS) {
        hsr_set_error("replay_plan: invalid sizes P=%d T=%d (P in 0..%d, T in 1..%d)", P, T, MAX_P, HSR_REPLAY_MAX_STEPS);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!out_upto || (P > 0 && !timestep)) {
        hsr_set_error("replay_plan: NULL out_upto, or NULL timestep with P=%d", P);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (bad_scratch("replay_plan", scratch, scratch_bytes, hsr_replay_plan_scratch_bytes(P, T))) return HSR_ERR_INVALID_ARGUMENT;
    unsigned* hist = reinterpret_cast<unsigned*>(scratch);
    HSR_HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)T * sizeof(unsigned), stream));
    if (P > 0) plan_hist_kernel<<<(P + RB - 1) / RB, RB, 0, stream>>>(P, T, timestep, hist);
    plan_scan_kernel<<<1, 1024, 0, stream>>>(T, hist, reinterpret_cast<long long*>(out_upto));
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" size_t hsr_replay_select_scratch_bytes(int P) { return hsr_align256(select_blocks(P) * sizeof(unsigned)); }

extern "C" int hsr_replay_select(int P, int S, int K, int transform_rots, int rot_source, int step, int capacity, const float* timestep,
                                 const float* means3D, const float* unnorm_rotations, const float* logit_opacities, const float* log_scales,
                                 const float* rgb_colors, const float* semantic, const float* w2c, float* out_means3D, float* out_unnorm_rot,
                                 float* out_rotations, float* out_opacities, float* out_scales, float* out_colors, float* out_semantic,
                                 int* out_index, int* out_count, char* scratch, size_t scratch_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || P > MAX_P || (S != 1 && S != 3) || K < 0 || K >= (1 << 23)) {
        hsr_set_error("replay_select: invalid sizes P=%d S=%d K=%d (P in 0..%d, log_scales must be [P,1] or [P,3], K in 0..%d)", P, S, K, MAX_P,
                      (1 << 23) - 1);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (rot_source != HSR_PREP_ROT_PARAMS && rot_source != HSR_PREP_ROT_TRANSFORMED) {
        hsr_set_error("replay_select: rot_source must be HSR_PREP_ROT_PARAMS or HSR_PREP_ROT_TRANSFORMED");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (transform_rots && !w2c) {
        hsr_set_error("replay_select: transform_rots needs w2c (16 floats, row-major, on the device)");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (capacity < 0 || !out_count) {
        hsr_set_error("replay_select: capacity=%d must not be negative and out_count not NULL", capacity);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const bool copy_sem = K > 0 && out_semantic;
    if (P > 0 && (!timestep || !means3D || !unnorm_rotations || !logit_opacities || !log_scales || !rgb_colors || (copy_sem && !semantic))) {
        hsr_set_error("replay_select: timestep, means3D, unnorm_rotations, logit_opacities, log_scales, rgb_colors (and semantic for "
                      "out_semantic with K > 0) are required");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (P > 0 && capacity > 0 && (!out_means3D || !out_rotations || !out_opacities || !out_scales || !out_colors)) {
        hsr_set_error("replay_select: an output pointer is NULL");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (bad_scratch("replay_select", scratch, scratch_bytes, hsr_replay_select_scratch_bytes(P))) return HSR_ERR_INVALID_ARGUMENT;
    unsigned* counts = reinterpret_cast<unsigned*>(scratch);
    const int nblk = (P + RB - 1) / RB;
    const float fstep = (float)step;
    if (P > 0) select_count_kernel<<<nblk, RB, 0, stream>>>(P, fstep, timestep, counts);
    select_scan_kernel<<<1, 1024, 0, stream>>>(nblk, counts, out_count);      // P == 0: writes the 0 and reads nothing
    if (P > 0 && capacity > 0) {
        ViewArgs a{P, S, transform_rots != 0, rot_source, means3D, unnorm_rotations, logit_opacities, log_scales, w2c};
        SelectOut o{out_means3D, out_unnorm_rot, out_rotations, out_opacities, out_scales, out_colors, copy_sem ? out_semantic : nullptr, out_index};
        if (w2c)
            select_emit_kernel<false><<<nblk, RB, 0, stream>>>(a, K, fstep, (unsigned)capacity, timestep, rgb_colors, semantic, counts, o);
        else
            select_emit_kernel<true><<<nblk, RB, 0, stream>>>(a, K, fstep, (unsigned)capacity, timestep, rgb_colors, semantic, counts, o);
    }
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_replay_cloud(int H, int W, const float* depth, const uint8_t* picture, float fx, float fy, float cx, float cy,
                                const float* c2w, float* out_points, uint8_t* out_records, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (hsr_bad_frame_size(H, W) || !depth || !c2w) {
        hsr_set_error("replay_cloud: invalid size H=%d W=%d or NULL depth / c2w", H, W);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!isfinite(fx) || !isfinite(fy) || fx == 0.f || fy == 0.f) {
        hsr_set_error("replay_cloud: fx and fy must be finite and not zero; got %g and %g", (double)fx, (double)fy);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if ((!out_points && !out_records) || (out_records && !picture)) {
        hsr_set_error("replay_cloud: out_points or out_records is required, and picture with out_records");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const long long N = (long long)H * W;
    const hsr_pinhole f{fx, fy, cx, cy};
    if (hsr_aligned(out_records, 4) && hsr_aligned(out_points, 4))
        cloud_kernel<4><<<(unsigned)(((N + 3) / 4 + RB - 1) / RB), RB, 0, stream>>>(N, W, depth, picture, f, c2w, out_points, out_records);
    else
        cloud_kernel<1><<<(unsigned)((N + RB - 1) / RB), RB, 0, stream>>>(N, W, depth, picture, f, c2w, out_points, out_records);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}
