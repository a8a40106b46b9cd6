// hsr_frame_export.hip — device export of one evaluated frame's pictures: float, label and logit maps to 8-bit R G B images, up to
// eight pictures in one launch (gfx950), DESIGN.md §7 row 9.  See include/ext/hsr_frame_export.h for the five rules, step by step, and
// the reference lines (utils/eval_helpers.py:92-133, :1314-1353, :1520-1537).
//   export_kernel<V> : blockIdx.y is the picture (its job struct is read from the kernel arguments with a wave-uniform index);
//                      V = 4: a lane takes 4 consecutive pixels of the flat index whatever W is — planar inputs and interleaved outputs
//                      are both contiguous over it — one 16-byte load per float or int32 plane (two for an int64 plane) and three dword
//                      stores per picture; the last H * W % 4 pixels go one at a time through the V = 1 path.  V = 1: a lane takes one
//                      pixel and stores three bytes, for calls with a src off 16 bytes or an out off 4.
// A plane of H * W % 4 != 0 floats puts the next plane off 16 bytes: the 16-byte accesses are declared 4-byte (8-byte for int64)
// aligned, which global memory takes at any dword (hsr_lane_io.h: the vector types and hsr_load<V>).  Streaming, bound by bytes: a
// 1200x680 frame with K = 26 logits and 4 levels reads 85 MB per LOGITS picture and writes 2.4 MB per picture; nothing is reused
// across lanes, so nothing is staged in LDS.  The LOGITS labels (hsr_tree.h's rule) read each plane of a level once for the maximum
// and once for the sum (the second read hits the caches).  Compiled with -ffp-contract=off: no rule of the header has a fused
// multiply-add.
#include <math.h>

#include "hsr_common.h"
#include "hsr_lane_io.h"
#include "hsr_tree.h"
#include "../../include/hsr_eval.h"
#include "../../include/ext/hsr_frame_resample.h"
#include "../../include/ext/hsr_frame_export.h"

namespace {

constexpr int XB = 256;

struct Jobs {
    hsr_export_job j[HSR_EXPORT_MAX_JOBS];
};

// V pixels from flat index i on: V = 4 packs the 12 bytes into three dwords (out is 4-byte aligned and i a multiple of 4)
template <int V> __device__ __forceinline__ void store(uint8_t* __restrict__ out, size_t i, const unsigned (&r)[V], const unsigned (&g)[V],
                                                        const unsigned (&b)[V]);
template <> __device__ __forceinline__ void store<1>(uint8_t* __restrict__ out, size_t i, const unsigned (&r)[1], const unsigned (&g)[1],
                                                     const unsigned (&b)[1])
{
    out[3 * i] = (uint8_t)r[0];
    out[3 * i + 1] = (uint8_t)g[0];
    out[3 * i + 2] = (uint8_t)b[0];
}
template <> __device__ __forceinline__ void store<4>(uint8_t* __restrict__ out, size_t i, const unsigned (&r)[4], const unsigned (&g)[4],
                                                     const unsigned (&b)[4])
{
    unsigned* __restrict__ w = reinterpret_cast<unsigned*>(out + 3 * i);
    w[0] = r[0] | g[0] << 8 | b[0] << 16 | r[1] << 24;
    w[1] = g[1] | b[1] << 8 | r[2] << 16 | g[2] << 24;
    w[2] = b[2] | r[3] << 8 | g[3] << 16 | b[3] << 24;
}

template <int V>
__device__ __forceinline__ void lookup(const uint8_t* __restrict__ table, const int (&idx)[V], const bool (&ok)[V], unsigned (&r)[V],
                                       unsigned (&g)[V], unsigned (&b)[V])
{
#pragma unroll
    for (int v = 0; v < V; v++) {
        r[v] = g[v] = b[v] = 0;
        if (ok[v]) {
            const uint8_t* __restrict__ row = table + 3 * (size_t)idx[v];
            r[v] = row[0]; g[v] = row[1]; b[v] = row[2];
        }
    }
}

// V pixels of picture `job` from flat index i on; N = H * W
template <int V>
__device__ __forceinline__ void export_pixels(const hsr_export_job& job, size_t i, size_t N)
{
    unsigned r[V], g[V], b[V];
    int idx[V];
    bool ok[V];
    if (job.kind == HSR_EXPORT_COLOR) {
        const float* __restrict__ src = static_cast<const float*>(job.src) + i;
        float x[3][V];
        hsr_load<V>(src, x[0]);
        hsr_load<V>(src + N, x[1]);
        hsr_load<V>(src + 2 * N, x[2]);
#pragma unroll
        for (int v = 0; v < V; v++) {
            r[v] = (unsigned)hsr_colour_code(x[0][v]);
            g[v] = (unsigned)hsr_colour_code(x[1][v]);
            b[v] = (unsigned)hsr_colour_code(x[2][v]);
        }
    } else if (job.kind == HSR_EXPORT_DEPTH) {
        float d[V];
        hsr_load<V>(static_cast<const float*>(job.src) + i, d);
        const float lo = job.lo, range = job.hi - job.lo;
#pragma unroll
        for (int v = 0; v < V; v++) {
            idx[v] = (int)(hsr_clamp01((d[v] - lo) / range) * 255.0f);
            ok[v] = true;
        }
        lookup<V>(job.table, idx, ok, r, g, b);
    } else if (job.kind == HSR_EXPORT_LABELS) {
        hsr_load<V>(static_cast<const int*>(job.src) + i, idx);
#pragma unroll
        for (int v = 0; v < V; v++) ok[v] = idx[v] >= 0 && idx[v] < job.n;
        lookup<V>(job.table, idx, ok, r, g, b);
    } else {
#pragma unroll
        for (int v = 0; v < V; v++) { idx[v] = 0; ok[v] = true; }
        if (job.kind == HSR_EXPORT_LEVELS) {
            const long long* __restrict__ src = static_cast<const long long*>(job.src) + i;
            for (int l = 0; l < job.L; l++) {
                long long lab[V];
                hsr_load<V>(src + (size_t)l * N, lab);
                const int size = job.sizes[l];
#pragma unroll
                for (int v = 0; v < V; v++) {
                    ok[v] = ok[v] && lab[v] >= 0 && lab[v] < (long long)size;
                    idx[v] = ok[v] ? idx[v] * size + (int)lab[v] : 0;      // < prod(sizes) = n while every label so far is in range
                }
            }
        } else {      // HSR_EXPORT_LOGITS
            const float* __restrict__ src = static_cast<const float*>(job.src) + i;
            int begin = 0;
            for (int l = 0; l < job.L; l++) {
                int lab[V];
                const int size = job.sizes[l];
                const float* __restrict__ x = src + (size_t)begin * N;      // hsr_tree.h's rule on V pixels: a 16-byte load per plane
                hsr_softmax_argmax<V>([&](int k, float (&t)[V]) { hsr_load<V>(x + (size_t)k * N, t); },
                                      [&](int k, int v) { return x[(size_t)k * N + v]; }, size, lab);
#pragma unroll
                for (int v = 0; v < V; v++) idx[v] = idx[v] * size + lab[v];
                begin += size;
            }
        }
        lookup<V>(job.table, idx, ok, r, g, b);
    }
    store<V>(job.out, i, r, g, b);
}

template <int V>
__global__ __launch_bounds__(XB) void export_kernel(Jobs jobs, long long N)
{
    const hsr_export_job& job = jobs.j[blockIdx.y];      // a wave-uniform index into the kernel arguments: scalar loads, no scratch
    const long long i = ((long long)blockIdx.x * XB + threadIdx.x) * V;
    if (i + V <= N) {
        export_pixels<V>(job, (size_t)i, (size_t)N);
    } else if (V > 1) {
        for (long long k = i; k < N; k++) export_pixels<1>(job, (size_t)k, (size_t)N);      // the last H * W % 4 pixels
    }
}

}  // namespace

extern "C" int hsr_frame_export(int H, int W, int n_jobs, const hsr_export_job* jobs, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (H < 1 || H > HSR_RESAMPLE_MAX_SIDE || W < 1 || W > HSR_RESAMPLE_MAX_SIDE) {
        hsr_set_error("frame_export: sides must be 1..%d; got %dx%d", HSR_RESAMPLE_MAX_SIDE, H, W);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (n_jobs < 1 || n_jobs > HSR_EXPORT_MAX_JOBS || !jobs) {
        hsr_set_error("frame_export: n_jobs must be 1..%d with a host array of that many jobs; got %d", HSR_EXPORT_MAX_JOBS, n_jobs);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    Jobs kj{};
    bool vec = true;
    for (int k = 0; k < n_jobs; k++) {
        const hsr_export_job& j = jobs[k];
        if (j.kind < HSR_EXPORT_COLOR || j.kind > HSR_EXPORT_LOGITS) {
            hsr_set_error("frame_export: job %d: unknown kind %d", k, j.kind);
            return HSR_ERR_INVALID_ARGUMENT;
        }
        if (!j.src || !j.out || (j.kind != HSR_EXPORT_COLOR && !j.table)) {
            hsr_set_error("frame_export: job %d (kind %d): NULL src, out or table", k, j.kind);
            return HSR_ERR_INVALID_ARGUMENT;
        }
        if (j.kind == HSR_EXPORT_DEPTH) {
            const float range = j.hi - j.lo;
            if (!isfinite(range) || !(range > 0.f)) {
                hsr_set_error("frame_export: job %d: hi - lo must be finite and positive; got lo %g hi %g", k, (double)j.lo, (double)j.hi);
                return HSR_ERR_INVALID_ARGUMENT;
            }
        }
        if ((j.kind == HSR_EXPORT_DEPTH && j.n != 256) || (j.kind == HSR_EXPORT_LABELS && j.n < 1)) {
            hsr_set_error("frame_export: job %d (kind %d): a table of %d rows; DEPTH takes 256, LABELS at least 1", k, j.kind, j.n);
            return HSR_ERR_INVALID_ARGUMENT;
        }
        if (j.kind == HSR_EXPORT_LEVELS || j.kind == HSR_EXPORT_LOGITS) {
            if (j.L < 1 || j.L > HSR_EVAL_MAX_LEVELS) {
                hsr_set_error("frame_export: job %d: L must be 1..%d; got %d", k, HSR_EVAL_MAX_LEVELS, j.L);
                return HSR_ERR_INVALID_ARGUMENT;
            }
            const hsr_tree_extent e = hsr_parse_tree_levels(j.L, j.sizes, nullptr);
            if (e.bad_level >= 0) {
                hsr_set_error("frame_export: job %d: level %d has %d classes", k, e.bad_level, j.sizes[e.bad_level]);
                return HSR_ERR_INVALID_ARGUMENT;
            }
            if (j.kind == HSR_EXPORT_LOGITS && e.sum > j.K) {
                hsr_set_error("frame_export: job %d: the levels need %lld planes, K is %d", k, e.sum, j.K);
                return HSR_ERR_INVALID_ARGUMENT;
            }
            if (e.prod != j.n) {
                hsr_set_error("frame_export: job %d: the levels need a table of %lld rows, n is %d", k, e.prod, j.n);
                return HSR_ERR_INVALID_ARGUMENT;
            }
        }
        vec = vec && hsr_aligned(j.src, 16) && hsr_aligned(j.out, 4);
        kj.j[k] = j;
    }
    const long long N = (long long)H * W;      // <= 2^28
    if (vec)
        export_kernel<4><<<dim3((unsigned)(((N + 3) / 4 + XB - 1) / XB), n_jobs), XB, 0, stream>>>(kj, N);
    else
        export_kernel<1><<<dim3((unsigned)((N + XB - 1) / XB), n_jobs), XB, 0, stream>>>(kj, N);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}
