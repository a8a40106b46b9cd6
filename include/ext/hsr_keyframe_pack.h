/*
 * hsr_keyframe_pack.h — C ABI of the keyframe store's packed form (libhsr_rast.so), DESIGN.md §7: a keyframe's float32 colour,
 * float32 depth and int64 label planes as 8-/16-bit codes, with a proof, from the same call, that the codes reproduce the planes bit
 * for bit.  The reference keeps every keyframe as float tensors (scripts/hierslam.py:2107-2124) and its checkpoint re-reads them from
 * the dataset (:1716-1752); a SLAM session that is to be saved and resumed keeps or writes them in this form (hsr_utils/checkpoint.py).
 * An extension under include/ext/: the prototypes under include/hsr_*.h are a counted set (tests/test_abi.py); these are bound under
 * this header's key in diff_gaussian_rasterization/_abi.py HEADERS.
 *
 * Why the codes can be exact: a frame that came through hsr_frame_ingest at sensor size has colour float(v) / 255.0f for an 8-bit v
 * and depth float(double(q) / depth_scale) for a 16-bit q (hsr_frame_ingest.h), and its labels are small non-negative integers.  The
 * packed form is 3 + 2 + 2 L bytes per pixel against 12 + 4 + 8 L.  Nothing is assumed: every value is checked, and the caller learns
 * how many did not survive.
 *
 * All pointers are DEVICE pointers and contiguous.  Everything runs on `stream`; nothing synchronises with the host, nothing
 * allocates, nothing is cleared beforehand.  N = H * W.  Errors: return <0 and hsr_last_error() (hsr_rasterizer.h).
 *
 * hsr_keyframe_pack — the rules, per value, in this order (the file is compiled with -ffp-contract=off):
 *   COLOUR  c = color[ch][i] (float32)
 *     t = c * 255.0f                                    one fp32 product
 *     v = rint(min(max(t, 0), 255))                     to nearest, halves to even; a NaN t gives 0
 *     out_color[ch][i] = uint8(v)
 *     exact iff bits(float(double(float(v)) / 255.0)) == bits(c)      the ingest's own expression applied to the code
 *   DEPTH   d = depth[i] (float32)
 *     t = double(d) * depth_scale                       one fp64 product
 *     q = rint(min(max(t, 0), 65535))                   a NaN t gives 0
 *     out_depth[i] = uint16(q)
 *     exact iff bits(float(double(q) / depth_scale)) == bits(d)       again the ingest's expression
 *   LABELS  l = labels[k][i] (int64)
 *     out_labels[k][i] = uint16(min(max(l, 0), 65535))
 *     exact iff 0 <= l <= 65535
 * The comparisons are on BIT PATTERNS: a NaN, an infinity, -0.0, a colour outside 0..1, a depth between two codes or beyond
 * 65535 / depth_scale and a negative label are all inexact, and nothing is undefined.  An inexact value still writes its clamped code.
 *   lossy[0] = the number of inexact colour values (of 3 N), lossy[1] of depth pixels (of N), lossy[2] of label values (of L N);
 *              a count that does not fit 32 bits (possible only for more than 2^32 - 1 inexact values) is stored as 2^32 - 1.
 * lossy is fully overwritten, 0 for an absent group.  The counts are made without atomics and without a clearing launch: every
 * workgroup of the pass leaves the count of its 1024 values in `scratch` and a one-workgroup finish adds them (the scheme of
 * hsr_view_holes): integers, so the result is exact and the same however it is reduced.
 * `color` and `depth` may each be NULL (the group is skipped; its output pointer is then not used); labels are given by L >= 1 with
 * both `labels` and `out_labels`, or absent with L == 0 and both NULL.  No output may overlap an input.
 * HSR_ERR_INVALID_ARGUMENT (-1), nothing launched, for: H or W outside 1 .. HSR_KEYFRAME_MAX_SIDE, L outside
 * 0 .. HSR_KEYFRAME_MAX_PLANES, a depth_scale that is zero or not finite, color without out_color, depth without out_depth, L >= 1
 * with labels or out_labels NULL, L == 0 with either not NULL, nothing to pack at all (color, depth NULL and L == 0), a NULL lossy, and
 * scratch that is NULL, smaller than hsr_keyframe_pack_scratch_bytes(H, W, L) or not 4-byte aligned.
 *
 * hsr_keyframe_unpack — the inverse, ONE launch, the same NULL rules (a group is given by its packed pointer):
 *     out_color[ch][i] = float(double(float(color_u8[ch][i])) / 255.0)
 *     out_depth[i]     = float(double(depth_u16[i]) / depth_scale)
 *     out_labels[k][i] = int64(labels_u16[k][i])
 * exactly the two expressions above (csrc/hsr_ingest_expr.h, which hsr_frame_ingest.hip writes its outputs with), so a group whose
 * lossy count was 0 comes back bit for bit.  The refusals are those of the pack without lossy and scratch.
 *
 * Both kernels stream: a lane takes 4 consecutive values of a plane's flat index — one 16-byte load per float plane, two per int64
 * plane, one 4-byte store for 4 colour codes, one 8-byte store for 4 16-bit codes — and the last N % 4 values of a plane go one at
 * a time; so does everything when a float or int64 base pointer is off 16 bytes, a uint8 one off 4 or a uint16 one off 8.
 */
#ifndef HSR_KEYFRAME_PACK_H_INCLUDED
#define HSR_KEYFRAME_PACK_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSR_KEYFRAME_MAX_SIDE 16384      /* HSR_RESAMPLE_MAX_SIDE: the sides the ingest produces */
#define HSR_KEYFRAME_MAX_PLANES 17       /* HSR_EVAL_MAX_LEVELS + 1: the tree levels and the leaf plane */

/* bytes of device scratch hsr_keyframe_pack needs: one 32-bit count per workgroup of the pass, (4 + L) planes of ceil(N / 1024) */
size_t hsr_keyframe_pack_scratch_bytes(int H, int W, int L);

/* color: float [3,H,W] or NULL; depth: float [H,W] or NULL; labels: int64 [L,H,W]; out_color: uint8 [3,H,W]; out_depth: uint16 [H,W];
 * out_labels: uint16 [L,H,W]; lossy: uint32 [3] */
int hsr_keyframe_pack(int H, int W, const float* color, const float* depth, int L, const int64_t* labels, double depth_scale,
                      uint8_t* out_color, uint16_t* out_depth, uint16_t* out_labels, uint32_t* lossy,
                      char* scratch, size_t scratch_bytes, void* stream);

int hsr_keyframe_unpack(int H, int W, const uint8_t* color_u8, const uint16_t* depth_u16, int L, const uint16_t* labels_u16,
                        double depth_scale, float* out_color, float* out_depth, int64_t* out_labels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSR_KEYFRAME_PACK_H_INCLUDED */
