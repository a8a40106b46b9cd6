/*
 * hsr_replay.h — C ABI of the replay of a finished run (libhsr_rast.so), DESIGN.md §7: the map as it stood at step t, ready for the
 * rasterizer, and a rendered view as a coloured world-space point cloud.  What the reference's viz_scripts/online_recon*.py and
 * final_recon.py do around their rasterizer calls for every step of a run: get_rendervars[_semantic]
 * (online_recon_sem_replica.py:100-158: `params['timestep'] <= curr_timestep`, a boolean index of every per-Gaussian tensor, then the
 * normalize / sigmoid / exp / tile chain) and rgbd2pcd (:220-259).  An extension under include/ext/: the prototypes under
 * include/hsr_*.h are a counted set (tests/test_abi.py); these are bound under this header's key in
 * diff_gaussian_rasterization/_abi.py HEADERS.
 *
 * All pointers are DEVICE pointers and contiguous; floats are fp32.  Everything runs on `stream`; nothing synchronises with the host
 * and nothing allocates.  Every refusal returns HSR_ERR_INVALID_ARGUMENT (-1) before any device work, with a message in
 * hsr_last_error() (hsr_rasterizer.h) that starts "replay_plan: ", "replay_select: " or "replay_cloud: ".  No kernel here waits for
 * another workgroup.
 *
 * hsr_replay_plan — once per run: how many Gaussians each step shows.
 *   out_upto[t] = #{ p : timestep[p] <= (float)t }      t = 0 .. T-1, fully overwritten (int64).
 * A row first shows at the smallest integer t >= timestep[p]: a negative or -inf timestep (and -0.0) at step 0, a fractional one at
 * its ceiling; a NaN, +inf or a value above T-1 never (the comparison is made in float BEFORE any conversion to an integer, so 1e30
 * does not wrap).  Two launches behind a clear of the bins: a T-bin integer histogram in `scratch` — one atomic per run of equal bins
 * within a wave, not one per row: rows come in long runs of equal timestep — and a one-workgroup scan turned inclusive.  Integers:
 * the result is the same in any order.  1 <= T <= HSR_REPLAY_MAX_STEPS; P == 0 is legal (timestep may be NULL) and gives zeros.
 * Refused: P < 0, T outside its range, a NULL out_upto, with P > 0 a NULL timestep, and scratch that is NULL, smaller than
 * hsr_replay_plan_scratch_bytes(P, T) (T 32-bit bins rounded up to 256 bytes) or not 4-byte aligned.
 *
 * hsr_replay_select — once per step: the rows with timestep[p] <= (float)step (a NaN is never selected), in their original order
 * (what the reference's boolean index yields, and what the per-tile sort's tie-break by row order needs), activated.  Output row r
 * comes from the r-th selected input row:
 *   out_means3D     w2c NULL: a bit copy of the row (the viz scripts keep the map in the world frame and give the pose to the
 *                   camera); w2c given (16 floats, row-major, on the device): hsr_view_prep's expression (hsr_view.h)
 *   out_unnorm_rot, out_rotations, out_opacities, out_scales
 *                   exactly hsr_view_prep's, from the same device function, with the same S, transform_rots and rot_source;
 *                   transform_rots needs w2c
 *   out_colors      [n,3] a bit copy of the rgb_colors row
 *   out_semantic    [n,K] a bit copy of the semantic row; K == 0 reads neither pointer
 *   out_index       [n] int32, the input row
 *   *out_count      the number of selected rows, whatever capacity is
 * Rows of rank >= capacity are not written.  out_unnorm_rot, out_semantic (also with K > 0) and out_index may be NULL.  Three
 * launches, the count / scan / emit of hsr_densify.h: 256-row blocks count, one workgroup scans the block counts, the emit recomputes
 * the rank.  The K columns are not copied a row per lane: the block leaves its destination rows in LDS and walks its 256 * K source
 * floats flat, so reads are coalesced and writes are wherever neighbours are both selected.  P == 0 writes *out_count = 0 in one
 * launch; capacity == 0 skips the emit.
 * Refused: P < 0, S not in {1, 3}, K < 0, an unknown rot_source, transform_rots with a NULL w2c, capacity < 0, a NULL out_count;
 * with P > 0 a NULL timestep, means3D, unnorm_rotations, logit_opacities, log_scales or rgb_colors, and with K > 0 and out_semantic
 * given a NULL semantic; with P > 0 and capacity > 0 a NULL out_means3D, out_rotations, out_opacities, out_scales or out_colors;
 * scratch that is NULL, smaller than hsr_replay_select_scratch_bytes(P) (one 32-bit count per 256 rows, rounded up to 256 bytes) or not
 * 4-byte aligned.
 *
 * hsr_replay_cloud — rgbd2pcd (:220-259) in ONE launch.  Pixel (x, y) with z = depth[y * W + x]:
 *   xx = (x - cx) / fx, yy = (y - cy) / fy, pc = (xx * z, yy * z, z),
 *   out[r] = ((c2w[4r] * pc0 + c2w[4r+1] * pc1) + c2w[4r+2] * pc2) + c2w[4r+3] * 1.0f      r = 0, 1, 2
 * each operation rounded once, in that order, no fused multiply-add (the chain of hsr_densify.h and hsr_map_init.h).  c2w is 16
 * floats, row-major, on the device.  EVERY pixel is emitted, as in the reference: zero depth lands on the camera centre.
 *   out_points      float32 [H*W,3]
 *   out_records     uint8 [H*W,15]: x, y, z as little-endian float32, then the pixel's R, G, B from `picture` (uint8 [H,W,3], a
 *                   hsr_frame_export picture): the body of a PLY file with property float x / y / z, uchar red / green / blue.
 * Either output may be NULL, not both; `picture` is required when out_records is given and not read otherwise.  A lane owns four
 * pixels (60 record bytes = 15 aligned dwords); a one-pixel variant with equal results takes the tail and every call whose out_records
 * is not 4-byte aligned.
 * Refused: H < 1, W < 1, H*W > 2^31-1, a NULL depth or c2w, both outputs NULL, out_records without picture, fx or fy zero or not finite.
 *
 * Not copied from the reference:
 *   - in render_mode='depth' rgbd2pcd re-normalises jet to each view's own maximum and paints depth >= 15 white; here a depth-coloured
 *     cloud takes hsr_frame_export's DEPTH picture, with the caller's lo and hi;
 *   - get_rendervars_semantic passes the UNSELECTED params['semantic'] beside selected rows (:154).  The rasterizer reads its first n
 *     rows, so the two agree exactly when the selection is a prefix of the map (every map the reference itself produces); otherwise the
 *     reference is wrong.  Here the semantic rows are selected like the rest.
 */
#ifndef HSR_REPLAY_H_INCLUDED
#define HSR_REPLAY_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#define HSR_REPLAY_MAX_STEPS (1 << 20)

#ifdef __cplusplus
extern "C" {
#endif

size_t hsr_replay_plan_scratch_bytes(int P, int T);

int hsr_replay_plan(int P, int T, const float* timestep, int64_t* out_upto,
                    char* scratch, size_t scratch_bytes, void* stream);

size_t hsr_replay_select_scratch_bytes(int P);

int hsr_replay_select(int P, int S, int K, int transform_rots, int rot_source, int step, int capacity,
                      const float* timestep, const float* means3D, const float* unnorm_rotations, const float* logit_opacities,
                      const float* log_scales, const float* rgb_colors, const float* semantic, const float* w2c,
                      float* out_means3D, float* out_unnorm_rot, float* out_rotations, float* out_opacities, float* out_scales,
                      float* out_colors, float* out_semantic, int* out_index, int* out_count,
                      char* scratch, size_t scratch_bytes, void* stream);

int hsr_replay_cloud(int H, int W, const float* depth, const uint8_t* picture, float fx, float fy, float cx, float cy,
                     const float* c2w, float* out_points, uint8_t* out_records, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSR_REPLAY_H_INCLUDED */
