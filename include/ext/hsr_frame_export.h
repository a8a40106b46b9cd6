/*
 * hsr_frame_export.h — C ABI of the device export of one evaluated frame's pictures (libhsr_rast.so), DESIGN.md §7 row 9: what the
 * reference's eval_*_newrender does between the float maps of a frame and cv2.imwrite (utils/eval_helpers.py:1520-1537 for the colour
 * and depth images, :1314-1353 with semantic_label_vis / semantic_label_vis_replica :92-133 for the semantic maps coloured per tree
 * tuple, :1054, :1070, :1335 for the maps coloured per class).  The mirror image of hsr_frame_ingest.h: float maps back to 8-bit
 * interleaved images, all of a frame's pictures in one launch.  An extension under include/ext/: the prototypes under include/hsr_*.h
 * are a counted set (tests/test_abi.py); this one is bound under its key in diff_gaussian_rasterization/_abi.py
 * HEADERS.
 *
 * One call is ONE launch for all n_jobs (1 .. HSR_EXPORT_MAX_JOBS) pictures of H x W pixels; the job structs travel by value in the
 * kernel's arguments.  No scratch, no allocation, no host synchronisation.  HSR_ERR_INVALID_ARGUMENT, and nothing launched, for: a
 * side outside 1 .. HSR_RESAMPLE_MAX_SIDE (16384, hsr_frame_resample.h), n_jobs outside 1..8 or jobs NULL, an unknown kind, a NULL
 * src or out, a NULL table for any kind but COLOR, n != 256 for DEPTH, n < 1 for LABELS, L outside 1 .. HSR_EVAL_MAX_LEVELS (16,
 * hsr_eval.h) for LEVELS and LOGITS, a level size below 1, sum(sizes) > K for LOGITS, prod(sizes) != n for LEVELS and LOGITS, and
 * hi - lo not finite or not positive for DEPTH.  No output may overlap an input or another output.  Fields a kind does not name are
 * not read.
 *
 * Every picture is uint8 [H,W,3] with the bytes R, G, B in memory.  cv2.imwrite takes B, G, R of the same colours (the reference
 * reverses its arrays before the call, or calls cv2.cvtColor), so a PNG written from these bytes by a library that takes R, G, B
 * (PIL) shows the reference's picture.  Tables are uint8 [n,3], rows R, G, B.  Nothing below needs a fused multiply-add; the file is
 * compiled with -ffp-contract=off so that none is formed.
 *
 * COLOR (:1520-1527, :1531-1536) — src float32 [3,H,W] planar.  Per value x:
 *     c = x > 0 ? (x < 1 ? x : 1) : 0          torch.clamp(x, 0, 1); a NaN gives 0
 *     p = c * 255.0f                           one fp32 product
 *     byte = p rounded to the nearest integer, halves to even
 * RESTATED, NOT PINNED BY cv2 (not available to this project's tests).  The rounding is believed to be that of imwrite's
 * convertTo(CV_8U) (cvRound, round half to even) from OpenCV's sources, NOT CHECKED.  torch.clamp keeps a NaN, which the reference
 * then hands to cvRound; that is believed to saturate to 0, NOT CHECKED — the 0 here is this header's statement.
 *
 * DEPTH (:1522-1526, :1533-1535) — src float32 [H,W], table [256,3] (the reference's is cv2.COLORMAP_JET), lo, hi (the reference:
 * 0 and 6).  With r = hi - lo, one fp32 subtraction on the host:
 *     n = (d - lo) / r                          one fp32 subtraction, one correctly rounded fp32 division
 *     n = n > 0 ? (n < 1 ? n : 1) : 0           np.clip; a NaN gives 0 (numpy's NaN -> uint8 is undefined, so it is stated here)
 *     idx = (int)(n * 255.0f)                   one fp32 product, truncated: astype(np.uint8) of a value in 0..255
 * The pixel is table[idx].  +inf gives table[255], -inf table[0].
 *
 * LABELS (:1054, :1070, :1335) — src int32 [H,W], table [n,3]: the pixel is table[label] for 0 <= label < n, else black (0, 0, 0).
 * The reference indexes a numpy array, whose negative indices wrap around to the end of the table; its labels there are never out
 * of range, and the wrap is deliberately NOT copied.
 *
 * LEVELS (semantic_label_vis*, on the ground-truth level planes that the ingest stores as int64) — src int64 [L,H,W], sizes[L],
 * table [n,3] with n = prod(sizes).  If 0 <= label_l < sizes[l] on every level l, compared in 64 bits (1 << 40 is out of range, not
 * wrapped),
 *     idx = (..((label_0 * sizes[1] + label_1) * sizes[2] + label_2)..) * sizes[L-1] + label_{L-1}
 * the mixed-radix index with level 0 most significant, exactly hsr_utils.evaluate.tree_lookup_table's, and the pixel is table[idx].
 * With any label out of range the pixel is black.  The per-key masks of the reference become one table over this index on the host
 * (hsr_utils.export.tuple_colour_table).
 *
 * LOGITS (:1314-1327) — src float32 [K,H,W], sizes[L], table [n,3] with n = prod(sizes).  Level l owns the planes
 * begin_l .. begin_l + sizes[l] - 1, begin_l = sizes[0] + .. + sizes[l-1]; planes from sum(sizes) on are not read.  The label of a
 * level is that of hsr_eval_labels_tree (hsr_eval.h), bit for bit (one definition, csrc/hsr_tree.h): with m the largest x_i of the level's planes (fmaxf from -inf, in
 * index order) and s the fp32 sum of expf(x_i - m) in index order, the lowest i with expf(x_i - m) / s == 1.0f / s; 0 when there is
 * none (a NaN or an infinity among the level's values).  Then as LEVELS (such labels are never out of range).
 *
 * All pointers are DEVICE pointers except `jobs`, a HOST array.  Everything runs on `stream`.  The kernel reads 16 bytes per plane and
 * lane and writes 12 per picture and lane (4 consecutive pixels of the flat index); when any src is not 16-byte aligned or any out
 * not 4-byte aligned the whole call takes a one-pixel-per-lane variant with the same results.  Errors: return <0 and hsr_last_error()
 * (hsr_rasterizer.h).
 */
#ifndef HSR_FRAME_EXPORT_H_INCLUDED
#define HSR_FRAME_EXPORT_H_INCLUDED

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSR_EXPORT_MAX_JOBS 8
#define HSR_EXPORT_COLOR   0   /* src float [3,H,W] planar                          -> out */
#define HSR_EXPORT_DEPTH   1   /* src float [H,W], table uint8 [256,3], lo, hi      -> out */
#define HSR_EXPORT_LABELS  2   /* src int32 [H,W], table uint8 [n,3]                -> out */
#define HSR_EXPORT_LEVELS  3   /* src int64 [L,H,W], sizes[L], table uint8 [prod,3] -> out */
#define HSR_EXPORT_LOGITS  4   /* src float [K,H,W], sizes[L], table uint8 [prod,3] -> out */

typedef struct hsr_export_job {
    int kind;
    const void* src;
    const uint8_t* table;
    int n;                        /* rows of table */
    int K, L;
    int sizes[16];                /* 16 = HSR_EVAL_MAX_LEVELS */
    float lo, hi;
    uint8_t* out;                 /* [H,W,3], R G B */
} hsr_export_job;

/* jobs: HOST array of n_jobs entries */
int hsr_frame_export(int H, int W, int n_jobs, const hsr_export_job* jobs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSR_FRAME_EXPORT_H_INCLUDED */
