/*
 * hsr_keyframes.h — C ABI of the mapping window's keyframe selection (libhsr_rast.so): what the reference runs for every mapped frame
 * (utils/keyframe_selection.py:40-96, keyframe_selection_overlap, called at scripts/hierslam.py:1966).
 *   valid pixels     torch.where(gt_depth[0] > 0) (:56-57) as a per-row prefix of the counts; the index list is never written
 *   sampled points   valid_depth_indices[indices] (:59), get_pointcloud's back-projection (:17-25) and its removal rule (:28-35)
 *   overlap counts   the per-keyframe projection and the five tests of :69-81, as integer counts for all keyframes at once
 * The random ranks (:58) and the permutation (:93) stay on the host generators (hsr_utils/keyframes.py).
 *
 * All pointers are DEVICE pointers unless marked host.  Everything runs on `stream` and nothing synchronises with the host.  Counts are
 * integers reduced in a fixed order: results are reproducible bit for bit.  Errors: return <0 and hsr_last_error() (hsr_rasterizer.h).
 * No allocation inside the library: callers pass scratch of at least the *_scratch_bytes size.
 */
#ifndef HSR_KEYFRAMES_H_INCLUDED
#define HSR_KEYFRAMES_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSR_KF_MAX_POINTS 4096   /* sample_points: ranks per call (their keys are compared in one workgroup's LDS) */

/* row_prefix (int32 [H+1], overwritten): row_prefix[r] = number of pixels with depth > 0 in rows [0, r) of depth ([H,W] fp32);
 * row_prefix[H] = n_valid, the bound of the reference's torch.randint (:58) — the 4 bytes the caller reads. */
int hsr_kf_valid_rows(int H, int W, const float* depth, int32_t* row_prefix, void* stream);

/* ranks (int64 [n], each in [0, n_valid)): rank r names the r-th pixel with depth > 0 in row-major order, which is what
 * valid_depth_indices[indices] yields (:56-59).  out_pixels (int32 [n,2]) receives its (row, col).  The point is get_pointcloud's
 * (:17-25), fp32 in this order: xx = (col - cx) / fx, yy = (row - cy) / fy, cam = (xx * z, yy * z, z),
 * pt_r = ((c2w[r][0] * cam_0 + c2w[r][1] * cam_1) + c2w[r][2] * cam_2) + c2w[r][3]   (c2w: 16 floats, row-major).
 * Removal rule (:28-35), the reference's as it stands: key = |nearbyint(pt * 1e4) / 1e4| per coordinate (torch.round(pts, decimals=4)
 * then abs); a point is removed when its key is (0, 0, 0) or equals the key of ANY OTHER sampled point — ranks are drawn with
 * replacement, so a pixel drawn twice loses all its copies.  out_keep (uint8 [n]): 1 = survives.  out_pts (float [n,3]): the survivors,
 * compacted in sampled order; out_count (int32 [1]): how many.  A rank outside [0, n_valid) gives pixel (-1, -1) and is removed.
 * 1 <= n <= HSR_KF_MAX_POINTS.  Scratch: hsr_kf_sample_scratch_bytes(n). */
size_t hsr_kf_sample_scratch_bytes(int n);
int hsr_kf_sample_points(int H, int W, const float* depth, const int32_t* row_prefix, int n, const int64_t* ranks, float fx, float fy,
                         float cx, float cy, const float* c2w, float* out_pts, int32_t* out_pixels, uint8_t* out_keep,
                         int32_t* out_count, char* scratch, size_t scratch_bytes, void* stream);

/* out_keys[i] = |nearbyint(vals[i] * 1e4) / 1e4|: the removal rule's key, element-wise over n floats (what sample_points compares). */
int hsr_kf_round_keys(int n, const float* vals, float* out_keys, void* stream);

/* out_counts[k] (int32 [n_kf], overwritten) = number of points of pts ([n_pts,3]) that pass all five tests of :79-81 in keyframe k:
 *   t_r = ((w2c_k[r][0] * x + w2c_k[r][1] * y) + w2c_k[r][2] * z) + w2c_k[r][3]              (:69-70; w2c: [n_kf,16] row-major)
 *   p_r = (intr[r][0] * t_0 + intr[r][1] * t_1) + intr[r][2] * t_2                         (:72; intr: 9 floats, the full product)
 *   zz = p_2 + 1e-5, u = p_0 / zz, v = p_1 / zz                                            (:74-76)
 *   u < W - edge, u > edge, v < H - edge, v > edge, zz > 0                                 (:78-81)
 * The number of points is n_pts, or *n_pts_dev clamped to [0, n_pts] when n_pts_dev != NULL (sample_points' out_count, so that the
 * host need not read it).  percent_inside (:83) is out_counts[k] / that number.  n_kf = 0 and n_pts = 0 are valid and launch nothing
 * (n_pts = 0 zero-fills out_counts). */
int hsr_kf_overlap_counts(int n_pts, const int32_t* n_pts_dev, const float* pts, int n_kf, const float* w2c, const float* intr, int W,
                          int H, int edge, int32_t* out_counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSR_KEYFRAMES_H_INCLUDED */
