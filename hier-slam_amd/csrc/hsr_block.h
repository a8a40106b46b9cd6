// hsr_block.h — workgroup primitives of the frame-sized helper units (internal, not part of the C ABI): wave and block sums, predicate
// counts, the order-preserving compaction rank, the single-workgroup exclusive scan, the fp32 chains several units share (pinhole
// back-projection, depth error) and the SSIM window.  Every device function is __device__ __forceinline__, so the including file's flags (-ffp-contract=off
// where the Makefile says so) apply to the inlined code.  Waves have 64 lanes; "block256" means exactly 256 threads in x (4 waves),
// "block1024" exactly 1024 (16 waves).  The rasterizer's hot path has its own tuned reductions (hsr_wave_reduce.h) and does not use these.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

// ---- waves -------------------------------------------------------------------------------------------------------------------
// xor butterfly 32, 16, ..., 1: every lane returns the wave's total (float, double, int, unsigned)
template <typename T>
__device__ __forceinline__ T hsr_wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// __shfl_up ladder 1, 2, ..., 32: lane l returns v[0] + ... + v[l]
template <typename T>
__device__ __forceinline__ T hsr_wave_inclusive_scan(T v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// ---- sums of a 256-thread block ----------------------------------------------------------------------------------------------
// Every thread returns ((s4[0] + s4[1]) + s4[2]) + s4[3], s4[w] being wave w's butterfly sum: that association order is the contract
// (loss values are pinned bit for bit).  A barrier precedes the store, so s4 may still be read by an earlier call; all threads call it.
__device__ __forceinline__ float hsr_block256_sum(float v, float* s4)
{
    v = hsr_wave_sum(v);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) s4[wv] = v;
    __syncthreads();
    return ((s4[0] + s4[1]) + s4[2]) + s4[3];
}

// N accumulators at once: one wave sum each, lane 0 to s[wave][k], then thread k < N writes out[k] = ((s[0][k] + s[1][k]) + s[2][k]) +
// s[3][k] — the same fixed order.  No leading barrier: s (4 rows) must be idle.  All threads call it.
template <int N, typename T>
__device__ __forceinline__ void hsr_block256_sums(const T (&v)[N], T (*s)[N], T* out)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; k++) {
        const T t = hsr_wave_sum(v[k]);
        if (lane == 0) s[wv][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const int k = threadIdx.x;
        out[k] = ((s[0][k] + s[1][k]) + s[2][k]) + s[3][k];
    }
}

// Integer total of a per-thread count; the result is valid in thread 0.  No leading barrier: s4 must be idle.  All threads call it.
template <typename T>
__device__ __forceinline__ T hsr_block256_isum(T c, T* s4)
{
    c = hsr_wave_sum(c);
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = c;
    __syncthreads();
    return s4[0] + s4[1] + s4[2] + s4[3];
}

// Number of threads with `pred` set; the result is valid in thread 0.  No leading barrier: s4 must be idle.  All threads call it.
__device__ __forceinline__ unsigned hsr_block256_count(bool pred, unsigned* s4)
{
    const unsigned long long b = __ballot(pred);
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = (unsigned)__popcll(b);
    __syncthreads();
    return s4[0] + s4[1] + s4[2] + s4[3];
}

// ---- order-preserving compaction ---------------------------------------------------------------------------------------------
// The number of threads with `pred` set and a lower threadIdx.x, in a block of WAVES waves; *total (if asked) receives the number of
// all threads with `pred` set.  Contains a barrier: EVERY thread of the workgroup calls it before any thread returns.  s_w: WAVES
// words, idle at the call; a caller that loops puts its own barrier before the next call.
template <int WAVES>
__device__ __forceinline__ unsigned hsr_block_rank(bool pred, unsigned* s_w, unsigned* total = nullptr)
{
    const unsigned long long b = __ballot(pred);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) s_w[w] = (unsigned)__popcll(b);
    __syncthreads();
    unsigned rank = (unsigned)__popcll(b & ((1ull << lane) - 1ull));
    if (total) {
        unsigned t = 0;
        for (int q = 0; q < WAVES; q++) { const unsigned v = s_w[q]; if (q < w) rank += v; t += v; }
        *total = t;
    } else {
        for (int q = 0; q < w; q++) rank += s_w[q];
    }
    return rank;
}

// ---- single-workgroup scan ---------------------------------------------------------------------------------------------------
// In place: counts[0, n) -> their exclusive prefix, for any n >= 0 (thread t owns the ceil(n / 1024) counts from t * ceil(n / 1024));
// every thread returns the total.  One workgroup of 1024 threads, all of which call it; s17: 17 words, idle at the call.  Contains two
// barriers; what a caller wrote to its own LDS before the call is visible to all threads after it.
template <typename T>
__device__ __forceinline__ T hsr_block1024_exclusive_scan(int n, T* __restrict__ counts, T* s17)
{
    const int per = (n + 1023) / 1024, beg = threadIdx.x * per;
    T local = 0;
    for (int k = 0; k < per; k++)
        if (beg + k < n) local += counts[beg + k];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const T inc = hsr_wave_inclusive_scan(local, lane);
    if (lane == 63) s17[w] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        T run = 0;
        for (int k = 0; k < 16; k++) { const T v = s17[k]; s17[k] = run; run += v; }
        s17[16] = run;
    }
    __syncthreads();
    T run = s17[w] + inc - local;
    for (int k = 0; k < per; k++)
        if (beg + k < n) { const T v = counts[beg + k]; counts[beg + k] = run; run += v; }
    return s17[16];
}

// ---- fp32 chains shared by densify, map init, keyframes and the masked loss -----------------------------------------------------
struct hsr_pinhole { float fx, fy, cx, cy; };

// get_pointcloud (scripts/hierslam.py:153-168, utils/keyframe_selection.py:17-25): xx = (x - CX) / FX, pts_cam = (xx * z, yy * z, z),
// pts = (c2w @ [pts_cam, 1])[:3].  The parentheses and the `* 1.0f` are the reference's evaluation order: means, log-scales and
// rounding keys decide bits from this chain, so the includers compile it with -ffp-contract=off.
__device__ __forceinline__ void hsr_backproject(float px, float py, float z, const hsr_pinhole& f, const float* __restrict__ c2w, float* out3)
{
    const float xx = (px - f.cx) / f.fx, yy = (py - f.cy) / f.fy;
    const float pc0 = xx * z, pc1 = yy * z, pc2 = z;
#pragma unroll
    for (int r = 0; r < 3; r++) out3[r] = ((c2w[4 * r] * pc0 + c2w[4 * r + 1] * pc1) + c2w[4 * r + 2] * pc2) + c2w[4 * r + 3] * 1.0f;
}

// scripts/hierslam.py:176-177: the depth over the mean focal length; its square is the new Gaussian's mean squared distance
__device__ __forceinline__ float hsr_depth_scale(float z, const hsr_pinhole& f) { return z / ((f.fx + f.fy) / 2.0f); }

// scripts/hierslam.py:911, in this order: |gt - d| * (gt > 0)
__device__ __forceinline__ float hsr_depth_error(float gt, float d) { return fabsf(gt - d) * (gt > 0.f ? 1.f : 0.f); }

// ---- the SSIM window of the loss head and of MS-SSIM ---------------------------------------------------------------------------
// gaussian(11, 1.5) as float32, normalised in float32 (utils/slam_external.py:54-56); built on the host, passed to the kernels by value.
// Each unit keeps its own 11-tap blur4 because the two round differently on purpose, and tests pin both: hsr_losses.hip runs an fmaf
// chain from 0 (the products are never rounded), hsr_msssim.hip is compiled with -ffp-contract=off and rounds every product and every
// sum once, in tap order, like the restatements its value is pinned against.
struct hsr_gauss { float g[11]; };

inline hsr_gauss hsr_gauss_window()
{
    hsr_gauss win;
    float sum = 0.f;
    for (int x = 0; x < 11; x++) {
        win.g[x] = (float)std::exp(-(double)((x - 5) * (x - 5)) / (2.0 * 1.5 * 1.5));
        sum += win.g[x];
    }
    for (int x = 0; x < 11; x++) win.g[x] = win.g[x] / sum;
    return win;
}
