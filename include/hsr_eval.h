/*
 * hsr_eval.h — C ABI of the per-frame map evaluation (libhsr_rast.so): what the reference computes for every
 * eval_every-th frame after mapping (utils/eval_helpers.py:1184-1630, eval_semantic_tree_newrender; flat semantics :869-1030).
 *   frame metrics    PSNR (calc_psnr, utils/slam_external.py:49-51), depth L1 and the "depth RMSE"        :1258-1295
 *   semantic labels  argmax(softmax) over all planes (flat), per tree level + the label_mapping_tree lookup
 *                    (transfer_tree_label :187-204, transfer_tree_2_label :135-156), or through the 1x1-conv leaf head (:1251-1255)
 *   IoU counts       calculate_iou (:83-90) and boundary_iou / mask_to_boundary (:37-81) for every class at once     :1297-1498
 *   per-frame score  mean IoU and mean boundary IoU over the classes present in the frame                          :1487-1498
 * The trajectory error (evaluate_ate / align, :218-275) is host numpy (hsr_utils/evaluate.py), not a kernel.
 *
 * All pointers are DEVICE pointers unless marked host; maps are planar CHW / HW, fp32 or int32.  Everything runs on `stream`
 * and nothing synchronises with the host.  Reductions are two-stage with a fixed order (floating sums) or integer (counts):
 * results are reproducible bit for bit.  Errors: return <0 and hsr_last_error() (hsr_rasterizer.h).  No allocation inside the
 * library: callers pass scratch of at least the *_scratch_bytes size.
 */
#ifndef HSR_EVAL_H_INCLUDED
#define HSR_EVAL_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSR_EVAL_MAX_CLASSES 4096   /* iou_counts: classes per call */
#define HSR_EVAL_MAX_LEVELS 16      /* tree labels: levels */
#define HSR_EVAL_LEAF_MAX_K 32      /* leaf labels: input planes */
#define HSR_EVAL_LEAF_MAX_C 256     /* leaf labels: classes */
#define HSR_EVAL_MAX_DILATION 1024  /* boundary IoU: erosion radius in pixels */

/* PSNR and depth errors of one frame (utils/eval_helpers.py:1258-1295).  im / gt_im: [3,H,W]; depth / gt_depth / final_opacity:
 * [H,W].  valid = gt_depth > 0; presence = final_opacity > sil_thres when final_opacity != NULL (the reference's
 * `mapping_iters == 0 and not add_new_gaussians` branch), else 1.  With rastered = depth * valid and e = (rastered - gt_depth) * presence:
 *   out3[0] = mean_c 20 log10(1 / sqrt(mse_c)),  mse_c = mean over all H*W pixels of (im_c*presence*valid - gt_c*presence*valid)^2
 *   out3[1] = sum |e| * valid / sum valid        out3[2] = sum sqrt(e*e) * valid / sum valid
 * out3: DEVICE double[3].  mse_c == 0 gives +inf, sum valid == 0 gives NaN, as in the reference. */
size_t hsr_eval_metrics_scratch_bytes(int H, int W);
int hsr_eval_frame_metrics(int H, int W, const float* im, const float* gt_im, const float* depth, const float* gt_depth,
                           const float* final_opacity, float sil_thres, double* out3, char* scratch, size_t scratch_bytes, void* stream);

/* Labels = argmax(softmax(logits)) per pixel: p_i = expf(x_i - max) / sum_j expf(x_j - max) in fp32, the FIRST index of the largest
 * p_i (ties among the probabilities, not the logits, go to the lowest index).  out_labels: int32 [H,W].
 * flat: over all K planes of `logits` ([K,H,W]). */
int hsr_eval_labels_flat(int K, int H, int W, const float* logits, int32_t* out_labels, void* stream);

/* tree: level l takes the channel range [sum(level_sizes[:l]), + level_sizes[l]) of `logits` (l < num_levels; level_sizes is a HOST
 * array — the dataset's num_semantic without its trailing leaf count).  out_level_labels (int32 [num_levels,H,W], may be NULL) receives
 * the per-level labels; out_labels the leaf id tree_table[mixed-radix index of the level labels] (tree_table: int32, prod(level_sizes)
 * entries, -1 where the tuple names no leaf; built on the host, hsr_utils/evaluate.py tree_lookup_table). */
int hsr_eval_labels_tree(int K, int H, int W, int num_levels, const int* level_sizes, const float* logits, const int32_t* tree_table,
                         int32_t* out_labels, int32_t* out_level_labels, void* stream);

/* leaf: logits_c = sum_k weight[c,k] * sem[k] + bias[c] (Conv2d(K, C, 1): weight [C,K], bias [C]), softmax over the C classes.  The
 * [C,H,W] logits are never written.  K <= HSR_EVAL_LEAF_MAX_K, C <= HSR_EVAL_LEAF_MAX_C.  Scratch: hsr_eval_leaf_scratch_bytes(C). */
size_t hsr_eval_leaf_scratch_bytes(int C);
int hsr_eval_labels_leaf(int K, int C, int H, int W, const float* sem, const float* weight, const float* bias, int32_t* out_labels,
                         char* scratch, size_t scratch_bytes, void* stream);

/* Per-class counts of one frame for C classes: out_counts (int64 [C,6], overwritten) row j = { G, P, I, G_b, P_b, I_b }:
 *   G = |gt == c_j|, P = |pred == c_j|, I = |gt == c_j and pred == c_j|, and the same over the boundary pixels of each map.
 * Classes: c_j = j when class_ids == NULL (C = num_classes); else the arbitrary int32 labels sorted_ids[0..C) (DEVICE, strictly
 * ascending) whose output rows are sorted_rows[0..C) (DEVICE int32, a permutation of 0..C-1).  A label in neither set counts for no
 * class.  Boundary (mask_to_boundary with the border padding of cv2.copyMakeBorder and `dilation` erosions of 3x3): a pixel is on the
 * boundary of its own class iff it lies within dilation-1 rows / columns of the image edge or a pixel within Chebyshev distance
 * `dilation` holds another label.  C <= HSR_EVAL_MAX_CLASSES, 1 <= dilation <= HSR_EVAL_MAX_DILATION.
 * pred / gt: int32 [H,W].  Scratch: hsr_eval_iou_scratch_bytes(H, W). */
size_t hsr_eval_iou_scratch_bytes(int H, int W);
int hsr_eval_iou_counts(int H, int W, const int32_t* pred, const int32_t* gt, int C, const int32_t* sorted_ids, const int32_t* sorted_rows,
                        int dilation, int64_t* out_counts, char* scratch, size_t scratch_bytes, void* stream);

/* out2 (DEVICE double[2]) = { mean over classes with G+P > 0 of I / (G+P-I), mean of I_b / (G_b+P_b-I_b) } from `counts` (int64
 * [C,6] as above).  No class present gives NaN, like np.mean([]). */
int hsr_eval_frame_miou(int C, const int64_t* counts, double* out2, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSR_EVAL_H_INCLUDED */
