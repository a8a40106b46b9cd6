/*
 * hsr_loss_outlier.h — C ABI of the outlier-rejecting loss head (libhsr_rast.so), DESIGN.md §7 row 2: the one branch of the
 * reference's get_loss* that include/hsr_losses.h leaves out, ignore_outlier_depth_loss = True (scripts/hierslam.py:909-937):
 *     depth_error = torch.abs(curr_data['depth'] - depth) * (curr_data['depth'] > 0)                                    :911
 *     mask = (depth_error < 10*depth_error.median())                                                                  :912
 *     mask = mask & (curr_data['depth'] > 0)                                                                          :913
 *     mask = mask & ~torch.isnan(depth)                     [& (silhouette > sil_thres) if tracking and use_sil_for_loss]   :916-919
 * with the masked depth and colour terms of :925-935.  An extension under include/ext/: the prototypes under include/hsr_*.h are a
 * counted set (tests/test_abi.py); this one is bound under its key in diff_gaussian_rasterization/_abi.py
 * HEADERS.  HSR_LOSS_SUM / HSR_LOSS_MEAN are those of hsr_losses.h.
 *
 * ERROR (:911).  e = fabsf(gt - d) * (gt > 0 ? 1.f : 0.f), in fp32, in that order, without contraction (csrc/hsr_loss_masked.hip, which
 * also holds hsr_loss_tracking_* of hsr_losses.h, is compiled with -ffp-contract=off).  NaN and inf travel as in torch: inf * 0 is NaN, and a NaN depth under a hole (gt <= 0) is still a NaN error.
 * fp32 denormals are kept, not flushed.  e is never negative, so its 32 bits order as an unsigned integer.
 *
 * MEDIAN (:912).  torch.median of all n = H * W errors: NaN if any e is NaN; otherwise the element of 0-based rank (n - 1) / 2
 * (integer division) in ascending order: with an even n the LOWER of the two middle values.  It is exact: a radix select over the
 * bits of e in three passes of 11, 11 and 10 bits.  Each pass is one launch in which every workgroup counts its pixels into a
 * histogram in LDS and adds its non-zero bins into a global one with integer atomics; the next launch begins with every workgroup
 * finding, in the finished global histogram, the bin that holds the rank.  The kernel boundary is the only synchronisation: no
 * workgroup reads within a launch what another wrote in it.  Integer arithmetic throughout: the median, the threshold and the count
 * are the same bits on every run.  No sort, no host read, no H * W-sized scratch, no mask tensor.
 *
 * THRESHOLD (:912).  threshold = 10.0f * median, one fp32 multiply.
 *
 * MASK (:912-919).  (e < threshold) & (gt > 0) & !isnan(d), and additionally & (silhouette > sil_thres) if use_sil.  The comparison
 * is strict; a NaN threshold selects nothing.
 *
 * TERMS (:925-935).  depth term = sum (HSR_LOSS_SUM, tracking :925) or mean (HSR_LOSS_MEAN, mapping :927) of |gt - d| over the mask;
 * colour term (C = 3) = sum of |gt_im - im| over the mask tiled on the channels, with or without the silhouette (:932-935), or with
 * HSR_LOSS_MEAN its mean over the tiled selection (the convention of hsr_loss_tracking_value).  C = 0 skips the colour term (im,
 * gt_im, d_im are then not read or written).  An empty selection gives sums of 0 and a mean of NaN, as torch's mean of an empty
 * selection; its gradients are 0 everywhere.
 *
 * GRADIENTS.  d_depth ([H,W]) / d_im ([C,H,W]) = upstream[0] * w * sign(pred - gt) on the selected pixels, additionally * 1/selected
 * (*inv_count, and / C for the colour) for the mean, and 0 elsewhere.  The mask is recomputed from *threshold, not stored.
 *
 * All pointers are DEVICE pointers; maps are planar CHW / HW, fp32, contiguous.  C is 0 or 3; H, W >= 1 and H * W < 2^31.
 * Everything runs on `stream`; nothing synchronises with the host.  No allocation inside the library.  Errors: return <0 and
 * hsr_last_error() (hsr_rasterizer.h), before anything is launched.
 *
 * SCRATCH.  hsr_loss_outlier_scratch_bytes(H, W) bytes of device memory (three histograms, a NaN counter, per-workgroup partial
 * sums; about 30 KB whatever the size).  Its contents need not be kept or cleared between calls: every call zeroes what it counts into.
 * Two calls in flight at once (two streams) need a scratch each.
 */
#ifndef HSR_LOSS_OUTLIER_H_INCLUDED
#define HSR_LOSS_OUTLIER_H_INCLUDED

#include <stddef.h>

#include "../hsr_losses.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t hsr_loss_outlier_scratch_bytes(int H, int W);

/* out2 (DEVICE float[2]) = { median, threshold } of depth / gt_depth ([H,W]).  Zeroing + 4 launches. */
int hsr_loss_outlier_median(int H, int W, const float* depth, const float* gt_depth, float* out2, char* scratch, size_t scratch_bytes,
                            void* stream);

/* Value pass.  out6 (DEVICE float[6]) = { depth term, colour term, w_depth * depth term + w_im * colour term, 1 / selected pixels,
 * median, threshold };  out_selected (DEVICE int[1]) = the number of selected pixels.  im / gt_im: [C,H,W]; depth / gt_depth /
 * silhouette: [H,W] (silhouette is read only if use_sil).  reduction: HSR_LOSS_SUM or HSR_LOSS_MEAN.  Zeroing + 5 launches: the
 * three histogram passes, the masked sums per workgroup, their fixed-order finish in double. */
int hsr_loss_outlier_value(int C, int H, int W, const float* im, const float* gt_im, const float* depth, const float* gt_depth,
                           const float* silhouette, float sil_thres, int use_sil, int reduction, float w_depth, float w_im, float* out6,
                           int* out_selected, char* scratch, size_t scratch_bytes, void* stream);

/* Gradient pass, one launch, when autograd asks.  threshold: &out6[5] of the value pass (DEVICE); upstream: DEVICE float, NULL = 1;
 * inv_count: &out6[3] of the value pass for HSR_LOSS_MEAN, NULL for sums; d_im ([C,H,W]) and d_depth ([H,W]): either may be NULL. */
int hsr_loss_outlier_grad(int C, int H, int W, const float* im, const float* gt_im, const float* depth, const float* gt_depth,
                          const float* silhouette, float sil_thres, int use_sil, float w_depth, float w_im, const float* threshold,
                          const float* upstream, const float* inv_count, float* d_im, float* d_depth, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSR_LOSS_OUTLIER_H_INCLUDED */
