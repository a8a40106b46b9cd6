/*
 * hsr_msssim.h — C ABI of the multi-scale SSIM of one evaluated frame (libhsr_rast.so): the `ms_ssim(...)` line of the reference's
 * per-frame evaluation (utils/eval_helpers.py:722, :946, :1272; masks :1259-1270), which the reference computes on the host after
 * copying both images there.  An extension of hsr_eval.h, in its own directory: the prototypes under include/hsr_*.h are a counted
 * set (tests/test_abi.py), these two are bound under this header's key in diff_gaussian_rasterization/_abi.py HEADERS.
 *
 * RESTATED, NOT PINNED BY THE REFERENCE'S PACKAGE: the reference calls pytorch_msssim.ms_ssim(data_range=1.0, size_average=True),
 * which is not available to this project's tests; the definition (Wang, Simoncelli, Bovik 2003) and that call's defaults are
 * restated below and checked against two independent float64 restatements (tests/msssim_ref.py).
 *
 * All pointers are DEVICE pointers; maps are planar CHW / HW, fp32.  Everything runs on `stream` and nothing synchronises with the
 * host.  Sums are two-stage with a fixed partition and order: results are reproducible bit for bit.  Errors: return <0 and
 * hsr_last_error() (hsr_rasterizer.h).  No allocation inside the library: callers pass scratch of at least the *_scratch_bytes size.
 */
#ifndef HSR_MSSSIM_H_INCLUDED
#define HSR_MSSSIM_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSR_EVAL_MSSSIM_SCALES 5
#define HSR_EVAL_MSSSIM_MIN_SIDE 161   /* min(H, W) >= this: the smaller side must exceed (11 - 1) * 2^4 */
#define HSR_EVAL_MSSSIM_OUT 31         /* doubles of `out`: 1 + 5 scales * 3 channels * 2 means */

/* MS-SSIM of one frame.  im / gt_im: [3,H,W]; gt_depth / final_opacity: [H,W].  Both images are multiplied by valid = gt_depth > 0
 * and, when final_opacity != NULL, by presence = final_opacity > sil_thres (im * presence * valid, as hsr_eval_frame_metrics) while
 * scale 0 is loaded; no masked copy is written.
 * Five scales, weights {0.0448, 0.2856, 0.3001, 0.2363, 0.1333}.  Per scale and channel, with the 11-tap Gaussian window of
 * sigma 1.5 (fp32, normalised by its sum; the window of hsr_loss_ssim) applied as a separable VALID filter (no padding: an h x w
 * image gives an (h-10) x (w-10) map) to x, y, x*x, y*y, x*y:
 *   s1 = E[xx] - m1*m1, s2 = E[yy] - m2*m2, s12 = E[xy] - m1*m2, C1 = 0.01^2, C2 = 0.03^2
 *   cs = (2 s12 + C2) / (s1 + s2 + C2),  ssim = (2 m1 m2 + C1) / (m1*m1 + m2*m2 + C1) * cs,  each averaged over the map.
 * Between scales both images pass a 2x2 average pool of stride 2 with zero padding of (size % 2) in front of each axis; padded
 * zeros count (the divisor is always 4).  With v_s = relu(mean cs) for the first four scales and relu(mean ssim) for the last,
 * the score of a channel is prod_s v_s^weight_s and the result the mean over the three channels.
 * out: DEVICE double[HSR_EVAL_MSSSIM_OUT]: out[0] the score; out[1 + (s*3 + c)*2 + {0, 1}] the means of cs and ssim of scale s,
 * channel c BEFORE relu.  min(H, W) < HSR_EVAL_MSSSIM_MIN_SIDE returns HSR_ERR_INVALID_ARGUMENT.
 * Scratch (hsr_eval_msssim_scratch_bytes(H, W)): pyramid levels 1..4 of both images and the per-tile partial sums.  The layout is
 * part of the contract (tests/msssim_ref.py scratch_layout restates it, tests/test_gpu_msssim_tiles.py reads it); with level 0 the
 * frame itself and h_s = (h_{s-1} + 1) / 2, w_s likewise:
 *   - from byte 0 the pyramid, fp32: for s = 1..4 in turn the x planes [3][h_s][w_s], then the y planes [3][h_s][w_s]; level s + 1
 *     is the 2x2 pool of level s evaluated as (((a00 + a01) + a10) + a11) * 0.25f, a_rc the window's row r and column c, each
 *     operation rounded once;
 *   - from the next 256-byte boundary the partial sums, double: [scale][tile_y * tiles_x + tile_x][channel][cs, ssim], the scales
 *     one after the other without gaps, with tiles_x = ceil((w_s - 10) / 32) and tiles_y = ceil((h_s - 10) / 32).  Tile (ty, tx)
 *     holds the sums of the two maps over rows [32 ty, min(32 ty + 32, h_s - 10)) and columns [32 tx, min(32 tx + 32, w_s - 10));
 *   - the size is that of the partials rounded up to 256 bytes as well.  Every pyramid pixel and every partial is written by each
 *     call, whatever the scratch held before, and nothing beyond the size is touched.
 * The means of `out` are the partials of a scale summed in double and divided by (h_s - 10)(w_s - 10). */
size_t hsr_eval_msssim_scratch_bytes(int H, int W);
int hsr_eval_msssim(int H, int W, const float* im, const float* gt_im, const float* gt_depth, const float* final_opacity,
                    float sil_thres, double* out, char* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSR_MSSSIM_H_INCLUDED */
