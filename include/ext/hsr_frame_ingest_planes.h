/*
 * hsr_frame_ingest_planes.h — C ABI of the device ingest of one raw sensor frame whose three images have SIZES OF THEIR OWN
 * (libhsr_rast.so), DESIGN.md §7 row 8.  A ScanNet frame is a 968x1296 colour JPEG, a 480x640 16-bit depth PNG and a 968x1296 16-bit
 * label-filt PNG (datasets/gradslam_datasets/scannet.py:404-418, :114); the reference resizes each of them once per size
 * (basedataset.py:223-227 and scripts/hierslam.py:1777 for the colour image, basedataset.py:248-256 for the depth map,
 * scannet.py:284-339 for the labels; scripts/hierslam.py:1543-1563 for the sizes).  hsr_frame_ingest.h takes one sensor size for all
 * three images; this entry takes one per image and is otherwise that entry: the same kernel runs behind both.  It reuses
 * hsr_ingest_level, HSR_INGEST_DEPTH_* and HSR_INGEST_MAX_LEVELS of hsr_frame_ingest.h.  An extension under include/ext/, bound under
 * its key in diff_gaussian_rasterization/_abi.py HEADERS (the header and the table of hsr_frame_ingest are pinned to that one name by
 * its suite).
 *
 * One call is ONE launch: an 8-bit interleaved colour image [Hc,Wc,3], a raw depth image [Hd,Wd] and, optionally, a raw class-id
 * image [Hl,Wl] become n_out (1 .. HSR_INGEST_MAX_LEVELS) levels of float32 planar colour in 0..1 and float32 depth in metres, plus,
 * at level 0's size only, the int64 label planes.  No scratch, no allocation, no host synchronisation.
 *
 * HSR_ERR_INVALID_ARGUMENT, and nothing launched, for:
 *   - n_out outside 1..3 or levels NULL;
 *   - Hc, Wc, Hd, Wd or a side of a level outside 1 .. HSR_RESAMPLE_MAX_SIDE (16384, hsr_frame_resample.h), each side checked on its
 *     own; Hl or Wl outside that range when labels is given (they are not read otherwise);
 *   - depth_type not one of the three HSR_INGEST_DEPTH_*; a depth_scale that is zero or not finite;
 *   - num_levels outside 0 .. HSR_EVAL_MAX_LEVELS (16, hsr_eval.h); leaf_column not 0 or 1; a table needed (num_levels > 0 or
 *     leaf_column) but NULL, or given with n_ids < 1;
 *   - out_labels NULL with labels given or the reverse, and any other NULL where a pointer is needed.
 * No output may overlap an input.
 *
 * RESTATED, NOT PINNED BY cv2: see hsr_frame_ingest.h; the same holds here.
 *
 * COLOUR — the rule of hsr_frame_ingest.h with (Hc, Wc) as the source: bilinear, half-pixel centres, replicated border, no
 * antialiasing, the taps in integers.  For destination column x of W columns
 *     n  = max((2x + 1) * Wc - W, 0)
 *     x0 = n / (2 * W)                         integer division: the left tap
 *     x1 = min(x0 + 1, Wc - 1)                 the right tap, clamped
 *     fx = double(n - x0 * 2 * W) / double(2 * W)
 * and the same for destination row y of H rows with Hc: y0, y1, fy.  With a = src[y0][x0][ch], b = src[y0][x1][ch],
 * c = src[y1][x0][ch], d = src[y1][x1][ch] converted from uint8 to double, in float64 and in this order, without fused multiply-add
 * (the file is compiled with -ffp-contract=off):
 *     top = a + fx * (b - a),   bot = c + fx * (d - c),   v = top + fy * (bot - top)
 * The output is float(v) / 255.0f (the reference's .type(torch.float) followed by / 255 on a float32 tensor).
 *
 * DEPTH — nearest, from its own (Hd, Wd): the source index is
 *     xs = (x * Wd) / W,   ys = (y * Hd) / H             integer division
 * and the output is float(double(raw[ys][xs]) / depth_scale), depth_scale being the reference's png_depth_scale (1000 for ScanNet).
 * raw is uint16, int32 or float32 (depth_type); with float32, NaN and inf travel through the division, and a zero stays a zero.
 * When the depth image already has a level's size (ScanNet's 480x640 depth at a 480x640 frame) the index is the identity, and the
 * bits of the quotient are what the equal-size case of hsr_frame_ingest gives.
 *
 * LABELS — written at level 0's size (H0, W0) only, nearest from their own (Hl, Wl):
 *     xs = (x * Wl) / W0,   ys = (y * Hl) / H0,   id = labels[ys][xs]
 * label_table is int32 [n_ids, num_levels + (leaf_column ? 1 : 0)], row-major.  With L = num_levels, known = (0 <= id < n_ids) and
 * row = label_table + id * (L + leaf_column):
 *     out[l][y][x] = known ? row[l] : id                       for l < L
 *     out[L][y][x] = (leaf_column && known) ? row[L] : id
 * With leaf_column == 0 this is the rule of hsr_frame_ingest.h: the last plane is the raw id.  With leaf_column == 1 the last plane
 * is the row's last column: the reference maps a raw ScanNet id to an NYU40 id, then to the tree levels, and keeps the NYU40 id as the
 * last plane (scannet.py:288-290, then :302-307 / :325-330 and the stack at :337-339); hsr_utils.frames.composed_label_table builds
 * the table of that composition.  An id the table does not hold keeps its raw value on every plane, as the reference's masked
 * assignments leave it.  leaf_column == 1 with num_levels == 0 is allowed: one plane, a flat remap (the reference's 'nyu40' mode,
 * scannet.py:288-290 alone).  The planes are int64, as in hsr_frame_ingest.h.
 *
 * All pointers are DEVICE pointers except `levels`, a HOST array whose structs are copied into the kernel's arguments by value.
 * Everything runs on `stream`.  Errors: return <0 and hsr_last_error() (hsr_rasterizer.h).
 */
#ifndef HSR_FRAME_INGEST_PLANES_H_INCLUDED
#define HSR_FRAME_INGEST_PLANES_H_INCLUDED

#include <stdint.h>

#include "hsr_frame_ingest.h"

#ifdef __cplusplus
extern "C" {
#endif

/* color_u8: [Hc,Wc,3] uint8; depth_raw: [Hd,Wd] of depth_type; labels: [Hl,Wl] int32 or NULL (Hl, Wl are then not read);
 * label_table: int32 [n_ids, num_levels + leaf_column], NULL when num_levels == 0 and leaf_column == 0 (n_ids is then not read);
 * levels: HOST array of n_out entries; out_labels: int64 [num_levels+1,H0,W0] at level 0's size, NULL exactly when labels is NULL
 * (num_levels, leaf_column, label_table and n_ids are then checked but not used). */
int hsr_frame_ingest_planes(int Hc, int Wc, const uint8_t* color_u8,
                            int Hd, int Wd, const void* depth_raw, int depth_type, double depth_scale,
                            int Hl, int Wl, const int* labels,
                            int num_levels, const int* label_table, int n_ids, int leaf_column,
                            int n_out, const hsr_ingest_level* levels, int64_t* out_labels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSR_FRAME_INGEST_PLANES_H_INCLUDED */
