// hsr_map_init.hip — first-frame map initialisation on device (gfx950), DESIGN.md §7 row 8.
// See include/ext/hsr_map_init.h for the reference lines (scripts/hierslam.py:419-578, :144-194, :322-409).
//   count : count_max_kernel — one count of depth > 0 and one maximum of depth per 256-pixel block;
//   scan  : scan_finish_kernel — one workgroup: exclusive scan of the block counts (total -> out_count) and the maximum of the
//           block maxima in a fixed order (-> out_scene_radius);
//   emit  : emit_rows_kernel — order-preserving compaction (block offset + wave ballot rank), back-projection, colours, log-scales,
//           identity rotations, zero opacities.
// The compaction is the one of hsr_densify.hip (block counts, single-workgroup scan, ballot rank).  Compiled with -ffp-contract=off:
// the emitted means are what the rasterizer will bin next, and means / scales stay comparable with a plain fp32 restatement.
#include "hsr_common.h"
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
    const unsigned long long b = __ballot(i < N && z > 0.f);
    const float m = wave_nan_max(z);
    if ((threadIdx.x & 63) == 0) { s_c[threadIdx.x >> 6] = (unsigned)__popcll(b); s_m[threadIdx.x >> 6] = m; }
    __syncthreads();
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = s_c[0] + s_c[1] + s_c[2] + s_c[3];
        bmax[blockIdx.x] = nan_max(nan_max(s_m[0], s_m[1]), nan_max(s_m[2], s_m[3]));
    }
}

__global__ __launch_bounds__(1024) void scan_finish_kernel(int nblk, unsigned* __restrict__ counts, const float* __restrict__ bmax,
                                                           float inv_ratio, int* __restrict__ out_count, float* __restrict__ out_radius)
{
    __shared__ unsigned s_w[17];
    __shared__ float s_m[16];
    const int per = (nblk + 1023) / 1024, beg = threadIdx.x * per;
    unsigned local = 0;
    float mx = -INFINITY;
    for (int k = 0; k < per; k++)
        if (beg + k < nblk) { local += counts[beg + k]; mx = nan_max(mx, bmax[beg + k]); }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned inc = local;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    mx = wave_nan_max(mx);
    if (lane == 63) s_w[w] = inc;
    if (lane == 0) s_m[w] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned run = 0;
        float m = s_m[0];
        for (int k = 0; k < 16; k++) { const unsigned v = s_w[k]; s_w[k] = run; run += v; m = nan_max(m, s_m[k]); }
        s_w[16] = run;
        *out_count = (int)run;
        if (out_radius) *out_radius = m * inv_ratio;
    }
    __syncthreads();
    unsigned run = s_w[w] + inc - local;
    for (int k = 0; k < per; k++)
        if (beg + k < nblk) { const unsigned v = counts[beg + k]; counts[beg + k] = run; run += v; }
}

struct Frame { float fx, fy, cx, cy; };

__global__ __launch_bounds__(MB) void emit_rows_kernel(const float* __restrict__ depth, const float* __restrict__ color, int W, int N, Frame f,
                                                       const float* __restrict__ c2w, const unsigned* __restrict__ offsets, int capacity, int S,
                                                       float* __restrict__ out_means, float* __restrict__ out_rgb,
                                                       float* __restrict__ out_log_scales, float* __restrict__ out_rots,
                                                       float* __restrict__ out_opac)
{
    __shared__ unsigned s_w[4];
    const int i = blockIdx.x * MB + threadIdx.x;
    const float z = i < N ? depth[i] : 0.f;
    const bool m = i < N && z > 0.f;
    const unsigned long long b = __ballot(m);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) s_w[w] = (unsigned)__popcll(b);
    __syncthreads();
    if (!m) return;
    unsigned pos = offsets[blockIdx.x] + (unsigned)__popcll(b & ((1ull << lane) - 1ull));
    for (int k = 0; k < w; k++) pos += s_w[k];
    if (pos >= (unsigned)capacity) return;
    // get_pointcloud (scripts/hierslam.py:153-168): xx = (x - CX)/FX, pts_cam = (xx*z, yy*z, z), pts = (c2w @ [pts_cam, 1])[:3]
    const int py = i / W, px = i - py * W;
    const float xx = ((float)px - f.cx) / f.fx, yy = ((float)py - f.cy) / f.fy;
    const float pc0 = xx * z, pc1 = yy * z, pc2 = z;
    const size_t row = pos;
#pragma unroll
    for (int r = 0; r < 3; r++)
        out_means[3 * row + r] = ((c2w[4 * r] * pc0 + c2w[4 * r + 1] * pc1) + c2w[4 * r + 2] * pc2) + c2w[4 * r + 3] * 1.0f;
#pragma unroll
    for (int c = 0; c < 3; c++) out_rgb[3 * row + c] = color[(size_t)c * N + i];
    const float sg = z / ((f.fx + f.fy) / 2.0f);   // :176-177
    const float ls = logf(sqrtf(sg * sg));         // :328-330, :387
    for (int c = 0; c < S; c++) out_log_scales[(size_t)S * row + c] = ls;
    out_rots[4 * row] = 1.0f;
    out_rots[4 * row + 1] = 0.f;
    out_rots[4 * row + 2] = 0.f;
    out_rots[4 * row + 3] = 0.f;
    out_opac[row] = 0.f;
}

size_t malign(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

extern "C" size_t hsr_map_init_scratch_bytes(int H, int W)
{
    if (H < 1 || W < 1) return 4096;
    const size_t nblk = ((size_t)H * W + MB - 1) / MB;
    return malign(nblk * sizeof(unsigned)) + malign(nblk * sizeof(float)) + 512;
}

extern "C" int hsr_map_init_frame(int H, int W, const float* depth, const float* color, float fx, float fy, float cx, float cy,
                                  const float* c2w, float scene_radius_depth_ratio, int capacity, int S, int* out_count, float* out_means3D,
                                  float* out_rgb, float* out_log_scales, float* out_unnorm_rotations, float* out_logit_opacities,
                                  float* out_scene_radius, char* scratch, size_t scratch_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (H < 1 || W < 1 || (size_t)H * W > 0x7fffffffu || !depth || !color || !c2w || !out_count) {
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
    if (!scratch || scratch_bytes < hsr_map_init_scratch_bytes(H, W)) {
        hsr_set_error("map_init_frame: scratch too small: %zu bytes needed", hsr_map_init_scratch_bytes(H, W));
        return HSR_ERR_BUFFER_TOO_SMALL;
    }
    const int N = H * W;
    const int nblk = (N + MB - 1) / MB;
    unsigned* counts = reinterpret_cast<unsigned*>(scratch);
    float* bmax = reinterpret_cast<float*>(scratch + malign((size_t)nblk * sizeof(unsigned)));
    count_max_kernel<<<nblk, MB, 0, stream>>>(depth, N, counts, bmax);
    scan_finish_kernel<<<1, 1024, 0, stream>>>(nblk, counts, bmax, 1.0f / scene_radius_depth_ratio, out_count, out_scene_radius);
    if (capacity > 0) {
        Frame f{fx, fy, cx, cy};
        emit_rows_kernel<<<nblk, MB, 0, stream>>>(depth, color, W, N, f, c2w, counts, capacity, S, out_means3D, out_rgb, out_log_scales,
                                                  out_unnorm_rotations, out_logit_opacities);
    }
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}
