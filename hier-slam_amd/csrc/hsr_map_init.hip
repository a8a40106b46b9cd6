// hsr_map_init.hip — first-frame map initialisation on device (gfx950), DESIGN.md §7 row 8.
// See include/ext/hsr_map_init.h for the reference lines (scripts/hierslam.py:419-578, :144-194, :322-409).
//   count : count_max_kernel — one count of depth > 0 and one maximum of depth per 256-pixel block;
//   scan  : scan_finish_kernel — one workgroup: exclusive scan of the block counts (total -> out_count) and the maximum of the
//           block maxima in a fixed order (-> out_scene_radius);
//   emit  : emit_rows_kernel — order-preserving compaction (block offset + wave ballot rank), back-projection, colours, log-scales,
//           identity rotations, zero opacities.
// The compaction is the one of hsr_densify.hip, from hsr_block.h (block counts, single-workgroup scan, ballot rank).  Compiled with
// -ffp-contract=off:
// the emitted means are what the rasterizer will bin next, and means / scales stay comparable with a plain fp32 restatement.
#include "hsr_common.h"
#include "hsr_block.h"
#include "../../include/ext/hsr_map_init.h"

#include <math.h>

namespace {

constexpr int MB = 256;

// torch.max: a NaN wins
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : fmaxf(a, b); }

__device__ __forceinline__ float wave_nan_max(float v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = nan_max(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(MB) void count_max_kernel(const float* __restrict__ depth, int N, unsigned* __restrict__ counts,
                                                       float* __restrict__ bmax)
{
    __shared__ unsigned s_c[4];
    __shared__ float s_m[4];
    const int i = blockIdx.x * MB + threadIdx.x;
    const float z = i < N ? depth[i] : -INFINITY;
    const float m = wave_nan_max(z);
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    const unsigned n = hsr_block256_count(i < N && z > 0.f, s_c);   // its barrier also publishes s_m
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = n;
        bmax[blockIdx.x] = nan_max(nan_max(s_m[0], s_m[1]), nan_max(s_m[2], s_m[3]));
    }
}

__global__ __launch_bounds__(1024) void scan_finish_kernel(int nblk, unsigned* __restrict__ counts, const float* __restrict__ bmax,
                                                           float inv_ratio, int* __restrict__ out_count, float* __restrict__ out_radius)
{
    __shared__ unsigned s_w[17];
    __shared__ float s_m[16];
    const int per = (nblk + 1023) / 1024, beg = threadIdx.x * per;   // the scan's partition
    float mx = -INFINITY;
    for (int k = 0; k < per; k++)
        if (beg + k < nblk) mx = nan_max(mx, bmax[beg + k]);
    mx = wave_nan_max(mx);
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = mx;
    const unsigned total = hsr_block1024_exclusive_scan(nblk, counts, s_w);   // its barriers also publish s_m
    if (threadIdx.x == 0) {
        float m = s_m[0];
        for (int k = 0; k < 16; k++) m = nan_max(m, s_m[k]);   // fixed order
        *out_count = (int)total;
        if (out_radius) *out_radius = m * inv_ratio;
    }
}

__global__ __launch_bounds__(MB) void emit_rows_kernel(const float* __restrict__ depth, const float* __restrict__ color, int W, int N, hsr_pinhole f,
                                                       const float* __restrict__ c2w, const unsigned* __restrict__ offsets, int capacity, int S,
                                                       float* __restrict__ out_means, float* __restrict__ out_rgb,
                                                       float* __restrict__ out_log_scales, float* __restrict__ out_rots,
                                                       float* __restrict__ out_opac)
{
    __shared__ unsigned s_w[4];
    const int i = blockIdx.x * MB + threadIdx.x;
    const float z = i < N ? depth[i] : 0.f;
    const bool m = i < N && z > 0.f;
    const unsigned rank = hsr_block_rank<4>(m, s_w);   // holds the barrier: no thread returns before it
    if (!m) return;
    const unsigned pos = offsets[blockIdx.x] + rank;
    if (pos >= (unsigned)capacity) return;
    const int py = i / W, px = i - py * W;
    const size_t row = pos;
    hsr_backproject((float)px, (float)py, z, f, c2w, out_means + 3 * row);
#pragma unroll
    for (int c = 0; c < 3; c++) out_rgb[3 * row + c] = color[(size_t)c * N + i];
    const float sg = hsr_depth_scale(z, f);
    const float ls = logf(sqrtf(sg * sg));         // :328-330, :387
    for (int c = 0; c < S; c++) out_log_scales[(size_t)S * row + c] = ls;
    out_rots[4 * row] = 1.0f;
    out_rots[4 * row + 1] = 0.f;
    out_rots[4 * row + 2] = 0.f;
    out_rots[4 * row + 3] = 0.f;
    out_opac[row] = 0.f;
}

}  // namespace

extern "C" size_t hsr_map_init_scratch_bytes(int H, int W)
{
    if (H < 1 || W < 1) return 4096;
    const size_t nblk = ((size_t)H * W + MB - 1) / MB;
    return hsr_align256(nblk * sizeof(unsigned)) + hsr_align256(nblk * sizeof(float)) + 512;
}

extern "C" int hsr_map_init_frame(int H, int W, const float* depth, const float* color, float fx, float fy, float cx, float cy,
                                  const float* c2w, float scene_radius_depth_ratio, int capacity, int S, int* out_count, float* out_means3D,
                                  float* out_rgb, float* out_log_scales, float* out_unnorm_rotations, float* out_logit_opacities,
                                  float* out_scene_radius, char* scratch, size_t scratch_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (hsr_bad_frame_size(H, W) || !depth || !color || !c2w || !out_count) {
        hsr_set_error("map_init_frame: invalid sizes H=%d W=%d or NULL depth/color/c2w/out_count", H, W);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (S != 1 && S != 3) {
        hsr_set_error("map_init_frame: S=%d; log_scales has 1 (isotropic) or 3 (anisotropic) columns", S);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (capacity < 0 || (capacity > 0 && (!out_means3D || !out_rgb || !out_log_scales || !out_unnorm_rotations || !out_logit_opacities))) {
        hsr_set_error("map_init_frame: capacity=%d needs out_means3D, out_rgb, out_log_scales, out_unnorm_rotations and out_logit_opacities",
                      capacity);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (int rc = hsr_check_scratch("map_init_frame", scratch, scratch_bytes, hsr_map_init_scratch_bytes(H, W))) return rc;
    const int N = H * W;
    const int nblk = (N + MB - 1) / MB;
    unsigned* counts = reinterpret_cast<unsigned*>(scratch);
    float* bmax = reinterpret_cast<float*>(scratch + hsr_align256((size_t)nblk * sizeof(unsigned)));
    count_max_kernel<<<nblk, MB, 0, stream>>>(depth, N, counts, bmax);
    scan_finish_kernel<<<1, 1024, 0, stream>>>(nblk, counts, bmax, 1.0f / scene_radius_depth_ratio, out_count, out_scene_radius);
    if (capacity > 0) {
        hsr_pinhole f{fx, fy, cx, cy};
        emit_rows_kernel<<<nblk, MB, 0, stream>>>(depth, color, W, N, f, c2w, counts, capacity, S, out_means3D, out_rgb, out_log_scales,
                                                  out_unnorm_rotations, out_logit_opacities);
    }
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}
