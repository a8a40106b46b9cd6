/*
 * hsr_map_init.h — C ABI of the first-frame map initialisation on device (libhsr_rast.so), DESIGN.md §7 row 8.
 *
 * Replaces, for frame 0, the numeric part of initialize_first_timestep / _semantic / _semantic_tree (scripts/hierslam.py:419-578):
 *     mask = depth > 0                                                                                     :446, :491, :557
 *     get_pointcloud(color, depth, intrinsics, w2c, mask=mask, compute_mean_sq_dist=True)                   :144-194
 *         xx = (x - CX) / FX, yy = (y - CY) / FY, pts_cam = (xx * z, yy * z, z), pts = (c2w @ [pts_cam, 1])[:3]
 *         mean3_sq_dist = (z / ((FX + FY) / 2))^2                                               ("projective")
 *     initialize_params / initialize_semantic_params                                                       :322-409
 *         log_scales = tile(log(sqrt(mean3_sq_dist)), S), unnorm_rotations = (1, 0, 0, 0), logit_opacities = 0
 *     scene_radius = max(depth) / scene_radius_depth_ratio                                                  :456, :503, :570
 * as ONE order-preserving stream compaction (row-major pixel order, exactly what `point_cld[mask]` yields): a per-block count and
 * maximum, one single-workgroup pass that scans the counts and finishes the maximum in a fixed order, and the ordered write.  No
 * full-frame point cloud, no boolean-mask gathers.
 *
 * The semantic rows are not produced here: the reference draws them with torch.rand (flag_init = 2, :363-376) and discards the
 * one-hot labels it computed.  The camera trajectory parameters and the bookkeeping vectors are zeros / constants made by torch.
 *
 * scene_radius is formed the way torch divides a device tensor by a host number: max(depth) * (1.0f / ratio).  A NaN depth is
 * never selected and makes scene_radius NaN, as torch.max does.
 *
 * All pointers are DEVICE pointers.  Errors: <0 and hsr_last_error().  No allocation inside the library.
 */
#ifndef HSR_MAP_INIT_H_INCLUDED
#define HSR_MAP_INIT_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t hsr_map_init_scratch_bytes(int H, int W);

/* depth: [H,W]; color: [3,H,W]; c2w: 16 floats row-major (inverse of the frame's w2c); S: columns of log_scales, 1 (isotropic) or 3
 * (anisotropic).  Outputs: out_count (int[1], the number of selected pixels M — may exceed `capacity`, in which case only the first
 * `capacity` rows are written), out_means3D [capacity,3], out_rgb [capacity,3], out_log_scales [capacity,S],
 * out_unnorm_rotations [capacity,4], out_logit_opacities [capacity,1], out_scene_radius float[1] (may be NULL).  capacity == 0
 * counts only (the row outputs may then be NULL). */
int hsr_map_init_frame(int H, int W, const float* depth, const float* color, float fx, float fy, float cx, float cy, const float* c2w,
                       float scene_radius_depth_ratio, int capacity, int S, int* out_count, float* out_means3D, float* out_rgb,
                       float* out_log_scales, float* out_unnorm_rotations, float* out_logit_opacities, float* out_scene_radius,
                       char* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSR_MAP_INIT_H_INCLUDED */
