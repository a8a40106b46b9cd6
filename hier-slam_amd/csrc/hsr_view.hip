// hsr_view.hip — the novel-view path (gfx950): rasterizer inputs from a GIVEN world-to-camera matrix, and the hole counts of a rendered
// view (include/ext/hsr_view.h).
//
// What it replaces in the reference, per view of eval_nvs (utils/eval_helpers.py:1692-1720, :1726-1738): the concatenation with a
// column of ones, the [4,4] @ [4,P] matmul and its slice, matrix_to_quaternion, two F.normalize and quat_mult, then the exp / sigmoid /
// F.normalize of transformed_params2rendervar (about a dozen launches) in front of the rasterizer; behind it a chain of boolean planes
// whose sum is read on the host for every view.
//
// view_prep_kernel is frame_prep_forward_kernel (hsr_frame_prep.hip) with R and t read from the matrix instead of built from a pose
// column: HBM-streaming, 36-44 B read and 44-60 B written per Gaussian, one thread per Gaussian, float4 access for the [P,4] rows.  The
// camera quaternion is computed by every thread from the 9 floats of the matrix (uniform loads, a few dozen VALU operations against
// ~100 B of traffic).  Compiled with -ffp-contract=off: out_means3D feeds the rasterizer's integer decisions and must be bit-equal to
// hsr_frame_prep_forward's for equal matrices.
// The per-row arithmetic is csrc/hsr_view_row.h's view_row(), which hsr_replay.hip runs as well with a selected row's rank as the destination.
// The hole counts are integers: a grid-stride pass with hsr_block.h's block sums, then a one-workgroup finish.
#include "hsr_common.h"
#include "hsr_block.h"
#include "hsr_view_row.h"
#include "../../include/ext/hsr_view.h"

namespace {

constexpr int VIEW_BLOCK = 256;
constexpr int HOLES_ITEMS = 4;         // pixels per thread and grid pass
constexpr int HOLES_MAX_BLOCKS = 96;   // workgroups of the pass: a frame of more than 96 * 1024 pixels takes further grid passes

__global__ __launch_bounds__(VIEW_BLOCK) void view_prep_kernel(ViewArgs a, float* __restrict__ out_means3D, float* __restrict__ out_unnorm_rot,
                                                               float* __restrict__ out_rotations, float* __restrict__ out_opacities,
                                                               float* __restrict__ out_scales)
{
    const int p = blockIdx.x * VIEW_BLOCK + threadIdx.x;
    if (p >= a.P) return;
    view_row<false>(a, (size_t)p, (size_t)p, out_means3D, out_unnorm_rot, out_rotations, out_opacities, out_scales);   // hsr_view_row.h
}

// partials[2 b], partials[2 b + 1]: the holes and the valid-depth pixels workgroup b saw (each below 2^31: N is)
__global__ __launch_bounds__(VIEW_BLOCK) void view_holes_kernel(const float* __restrict__ sil, const float* __restrict__ gt_depth, float sil_thres,
                                                                unsigned N, unsigned* __restrict__ partials)
{
    __shared__ unsigned s_red[VIEW_BLOCK / 64][2];
    unsigned c[2] = {0u, 0u};
    const size_t pass = (size_t)gridDim.x * VIEW_BLOCK * HOLES_ITEMS;
    for (size_t base = (size_t)blockIdx.x * VIEW_BLOCK * HOLES_ITEMS + threadIdx.x; base < N; base += pass) {
#pragma unroll
        for (int it = 0; it < HOLES_ITEMS; it++) {
            const size_t i = base + (size_t)it * VIEW_BLOCK;
            if (i < N) {
                const bool valid = gt_depth[i] > 0.f;
                c[0] += (valid && !(sil[i] > sil_thres)) ? 1u : 0u;
                c[1] += valid ? 1u : 0u;
            }
        }
    }
    hsr_block256_sums(c, s_red, partials + 2 * (size_t)blockIdx.x);
}

__global__ __launch_bounds__(VIEW_BLOCK) void view_holes_finish_kernel(const unsigned* __restrict__ partials, int nblocks, long long* __restrict__ out2)
{
    __shared__ long long s_red[VIEW_BLOCK / 64][2];
    long long c[2] = {0, 0};
    for (int b = threadIdx.x; b < nblocks; b += VIEW_BLOCK) { c[0] += partials[2 * b]; c[1] += partials[2 * b + 1]; }
    hsr_block256_sums(c, s_red, out2);
}

int holes_blocks(int H, int W)
{
    const size_t per = (size_t)VIEW_BLOCK * HOLES_ITEMS;
    const size_t nb = ((size_t)H * W + per - 1) / per;
    return (int)(nb < (size_t)HOLES_MAX_BLOCKS ? nb : (size_t)HOLES_MAX_BLOCKS);
}

}  // namespace

extern "C" int hsr_view_prep(int P, int S, int transform_rots, int rot_source, const float* means3D, const float* unnorm_rotations,
                             const float* logit_opacities, const float* log_scales, const float* w2c, float* out_means3D,
                             float* out_unnorm_rot, float* out_rotations, float* out_opacities, float* out_scales, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || (S != 1 && S != 3)) {
        hsr_set_error("view_prep: invalid sizes P=%d S=%d (log_scales must be [P,1] or [P,3])", P, S);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (rot_source != HSR_PREP_ROT_PARAMS && rot_source != HSR_PREP_ROT_TRANSFORMED) {
        hsr_set_error("view_prep: rot_source must be HSR_PREP_ROT_PARAMS or HSR_PREP_ROT_TRANSFORMED");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!w2c) {
        hsr_set_error("view_prep: w2c is required (16 floats, row-major, on the device)");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (P == 0) return HSR_OK;
    if (!means3D || !unnorm_rotations || !logit_opacities || !log_scales) {
        hsr_set_error("view_prep: means3D, unnorm_rotations, logit_opacities and log_scales are required");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!out_means3D || !out_rotations || !out_opacities || !out_scales) {
        hsr_set_error("view_prep: an output pointer is NULL");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    ViewArgs a{P, S, transform_rots != 0, rot_source, means3D, unnorm_rotations, logit_opacities, log_scales, w2c};
    view_prep_kernel<<<(P + VIEW_BLOCK - 1) / VIEW_BLOCK, VIEW_BLOCK, 0, stream>>>(a, out_means3D, out_unnorm_rot, out_rotations,
                                                                                  out_opacities, out_scales);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" size_t hsr_view_holes_scratch_bytes(int H, int W)
{
    if (hsr_bad_frame_size(H, W)) return 1024;
    return hsr_align256((size_t)holes_blocks(H, W) * 2 * sizeof(unsigned));
}

extern "C" int hsr_view_holes(int H, int W, const float* silhouette, const float* gt_depth, float sil_thres, int64_t* out2, char* scratch,
                              size_t scratch_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (hsr_bad_frame_size(H, W) || !silhouette || !gt_depth || !out2) {
        hsr_set_error("view_holes: invalid size H=%d W=%d or NULL silhouette / gt_depth / out2", H, W);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const size_t need = hsr_view_holes_scratch_bytes(H, W);
    if (!scratch || scratch_bytes < need || (reinterpret_cast<uintptr_t>(scratch) & 3) != 0) {
        hsr_set_error("view_holes: scratch too small: %zu bytes needed, %zu given (or NULL, or not 4-byte aligned)", need, scratch_bytes);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const int nb = holes_blocks(H, W);
    unsigned* partials = reinterpret_cast<unsigned*>(scratch);
    view_holes_kernel<<<nb, VIEW_BLOCK, 0, stream>>>(silhouette, gt_depth, sil_thres, (unsigned)((size_t)H * W), partials);
    view_holes_finish_kernel<<<1, VIEW_BLOCK, 0, stream>>>(partials, nb, reinterpret_cast<long long*>(out2));
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}
