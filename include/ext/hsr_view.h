/*
 * hsr_view.h — C ABI of the novel-view path (libhsr_rast.so), DESIGN.md §7: the map rendered from a GIVEN world-to-camera matrix
 * instead of a column of the pose parameters, and the hole count that decides whether such a view is scored.  What the reference's
 * eval_nvs runs per view around its two rasterizer calls (utils/eval_helpers.py:1692-1720 in front, :1726-1738 behind), and what its
 * viz_scripts do before they draw (get_rendervars(params, w2c, ...)).  An extension under include/ext/: the prototypes under
 * include/hsr_*.h are a counted set (tests/test_abi.py); these are bound under this header's key in
 * diff_gaussian_rasterization/_abi.py HEADERS.
 *
 * All pointers are DEVICE pointers, fp32 (out2: int64) and contiguous.  Everything runs on `stream`; nothing synchronises with the
 * host and nothing allocates.  Errors: return <0 and hsr_last_error() (hsr_rasterizer.h).
 *
 * hsr_view_prep — ONE launch, one thread per Gaussian, forward only (a novel view is never optimised).  `w2c` is 16 floats,
 * row-major, ON THE DEVICE: the kernel reads it, so a pose computed on the device costs no copy.  Restated from eval_nvs :1692-1712
 * and transformed_params2rendervar[_semantic] (utils/slam_helpers.py:124-139, :195-219), all fp32:
 *   out_means3D[p][i]  = ((x * w2c[4i] + y * w2c[4i+1]) + z * w2c[4i+2]) + w2c[4i+3]      i = 0, 1, 2, in that order, no fused
 *                        multiply-add: the expression of hsr_frame_prep_forward with R = w2c[:3,:3] and t = w2c[:3,3], so equal
 *                        matrices give equal bits (out_means3D feeds the rasterizer's integer decisions).  With the identity the
 *                        output is means3D bit for bit (for finite values; a -0.0 comes out as +0.0 where a +0.0 product is added).
 *   q                  = F.normalize(matrix_to_quaternion(w2c[:3,:3]))    only with transform_rots; computed in the kernel from the 9
 *                        floats (uniform over the launch): the pivots 1+m00+m11+m22, 1+m00-m11-m22, 1-m00+m11-m22, 1-m00-m11+m22
 *                        summed left to right, the LARGEST decides the branch and the first wins ties (argmax), its row of
 *                        {pivot, m21-m12, m02-m20, m10-m01 | m21-m12, pivot, m10+m01, m02+m20 | m02-m20, m10+m01, pivot, m21+m12 |
 *                        m10-m01, m02+m20, m21+m12, pivot} divided by 2 * sqrt(max(pivot, 1e-12)), negated when its real part is
 *                        negative (hsr_utils/slam.py matrix_to_quaternion); then x / max(|x|, 1e-12).
 *   out_unnorm_rot[p]  = transform_rots ? quat_mult(q, F.normalize(unnorm_rotations[p])) : unnorm_rotations[p] (a bit copy)
 *   out_rotations[p]   = F.normalize(rot_source == HSR_PREP_ROT_PARAMS ? unnorm_rotations[p] : out_unnorm_rot[p])
 *   out_opacities[p]   = sigmoid(logit_opacities[p])
 *   out_scales[p,0..2] = exp(log_scales[p, S == 1 ? 0 : 0..2])
 * S, rot_source (HSR_PREP_ROT_PARAMS = 0 / HSR_PREP_ROT_TRANSFORMED = 1) and the last four outputs are exactly those of
 * include/hsr_frame_prep.h, from the same expressions (csrc/hsr_quat.h); the reference sets transform_rots iff S == 3.  out_unnorm_rot
 * may be NULL.  P == 0 is legal and launches nothing (its array pointers may be NULL).  HSR_ERR_INVALID_ARGUMENT (-1), nothing
 * launched, for P < 0, S not in {1, 3}, an unknown rot_source, a NULL w2c, and with P > 0 a NULL among means3D, unnorm_rotations,
 * logit_opacities, log_scales, out_means3D, out_rotations, out_opacities, out_scales.
 *
 * hsr_view_holes — the two integer counts behind eval_nvs's percent_holes (:1726-1734), over the H*W pixels:
 *   out2[0] = #{ !(silhouette > sil_thres) && gt_depth > 0 }      a NaN silhouette is a hole (NaN > t is false); a NaN or negative
 *   out2[1] = #{ gt_depth > 0 }                                    gt_depth is not valid
 * A grid-stride pass leaves one pair of counts per workgroup in `scratch` and a one-workgroup finish adds them: integers, so the
 * result is exact and the same however it is reduced.  out2 is fully overwritten; the caller clears nothing.
 * HSR_ERR_INVALID_ARGUMENT (-1), nothing launched, for H < 1, W < 1, H*W > 2^31-1, a NULL silhouette, gt_depth or out2, and for
 * scratch that is NULL, smaller than hsr_view_holes_scratch_bytes(H, W) or not 4-byte aligned.
 */
#ifndef HSR_VIEW_H_INCLUDED
#define HSR_VIEW_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int hsr_view_prep(int P, int S, int transform_rots, int rot_source,
                  const float* means3D, const float* unnorm_rotations,
                  const float* logit_opacities, const float* log_scales,
                  const float* w2c,
                  float* out_means3D, float* out_unnorm_rot, float* out_rotations,
                  float* out_opacities, float* out_scales, void* stream);

/* bytes of device scratch hsr_view_holes needs (one pair of counts per workgroup of the pass) */
size_t hsr_view_holes_scratch_bytes(int H, int W);

int hsr_view_holes(int H, int W, const float* silhouette, const float* gt_depth, float sil_thres,
                   int64_t* out2, char* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSR_VIEW_H_INCLUDED */
