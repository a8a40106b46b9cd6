/*
 * hsr_frame_ingest.h — C ABI of the device ingest of one raw sensor frame (libhsr_rast.so), DESIGN.md §7 row 8: what the reference's
 * dataset objects do between a decoded image and the frame loop (datasets/gradslam_datasets/basedataset.py:223-227 and
 * scripts/hierslam.py:1777 for the colour image, basedataset.py:248-256 for the depth map, replica.py:241-299 and :369 for the labels),
 * once per size when tracking and densification have sizes of their own (scripts/hierslam.py:1543-1563).  An extension under
 * include/ext/: the prototypes under include/hsr_*.h are a counted set (tests/test_abi.py); this one is bound under its key in
 * diff_gaussian_rasterization/_abi.py HEADERS.
 *
 * One call is ONE launch: an 8-bit interleaved colour image, a raw depth image and, optionally, a raw class-id image, all at the
 * sensor size Hs x Ws (hsr_frame_ingest_planes.h: the same with a size per image, and a leaf column in the label table), become n_out (1 .. HSR_INGEST_MAX_LEVELS) levels of float32 planar colour in 0..1 and float32 depth in
 * metres, plus, at level 0's size only, one int64 label plane per tree level and one for the raw id.  No scratch, no allocation, no
 * host synchronisation.  Sides (the sensor's and every level's) are 1 .. HSR_RESAMPLE_MAX_SIDE (16384, hsr_frame_resample.h).
 * HSR_ERR_INVALID_ARGUMENT, and nothing launched, for: a side outside that range, n_out outside 1..3, depth_type not one of the
 * three below, num_levels outside 0 .. HSR_EVAL_MAX_LEVELS (16, hsr_eval.h), num_levels > 0 without a table or with n_ids < 1, a depth_scale that is zero or not finite, out_labels NULL with labels given or the reverse, and any other NULL where a
 * pointer is needed.  No output may overlap an input.
 *
 * RESTATED, NOT PINNED BY cv2: the reference resizes with cv2.resize, which is not available to this project's tests.  The
 * reference reads the image with dtype=float (basedataset.py:298, replica.py:381), so cv2 interpolates in float64 on the values
 * 0..255 and rounds to no grey level; the rule below does the same.  One known difference is believed from OpenCV's sources and
 * NOT CHECKED here: cv2's float64 INTER_LINEAR path keeps its interpolation weights in fp32; if so, its values differ from the
 * ones below by about 255 * 2^-24 grey levels (1.5e-5 of a grey level, 6e-8 of the 0..1 range).
 *
 * COLOUR — bilinear, half-pixel centres, replicated border, no antialiasing.  The taps are those of hsr_frame_resample.h, in
 * integers: for destination column x of Wd columns from Ws source columns
 *     n  = max((2x + 1) * Ws - Wd, 0)
 *     x0 = n / (2 * Wd)                        integer division: the left tap
 *     x1 = min(x0 + 1, Ws - 1)                 the right tap, clamped
 *     fx = double(n - x0 * 2 * Wd) / double(2 * Wd)
 * and the same for destination row y with Hs, Hd: y0, y1, fy.  With a = src[y0][x0][ch], b = src[y0][x1][ch], c = src[y1][x0][ch],
 * d = src[y1][x1][ch] converted from uint8 to double, in float64 and in this order, without fused multiply-add (the file is
 * compiled with -ffp-contract=off):
 *     top = a + fx * (b - a),   bot = c + fx * (d - c),   v = top + fy * (bot - top)
 * The output is float(v) / 255.0f: v rounded to fp32, then one correctly rounded fp32 division — the reference's .type(torch.float)
 * followed by / 255 on a float32 tensor.  (float(double(float(v)) / 255.0) is the same value: the double quotient of two floats
 * rounds to the same float.)  Equal sizes give fx = fy = 0, so each value is float(g) / 255.0f exactly.
 *
 * DEPTH — nearest: the source index is
 *     xs = (x * Ws) / Wd,   ys = (y * Hs) / Hd          integer division
 * and the output is float(double(raw[ys][xs]) / depth_scale), depth_scale being the reference's png_depth_scale.  raw is uint16,
 * int32 or float32 (depth_type); with float32, NaN and inf travel through the division, and a zero stays a zero.
 *
 * LABELS — written at level 0's size only (nothing at a reduced size reads labels): the nearest index is the depth's,
 * id = labels[ys][xs], and with L = num_levels
 *     out[l][y][x] = tree_table[id * L + l]  if 0 <= id < n_ids, else id          for l < L
 *     out[L][y][x] = id
 * A class the table does not know keeps its raw id on every level, as the reference's masked assignments on copies of the raw image
 * leave it (replica.py:235-247).  With L = 0 the single plane is the resized id image (flat classes).  The planes are int64
 * because every loss head converts its labels to int64 each iteration; a stored int64 plane makes that a no-op.
 *
 * All pointers are DEVICE pointers except `levels`, a HOST array whose structs are copied into the kernel's arguments by value.
 * Everything runs on `stream`.  Errors: return <0 and hsr_last_error() (hsr_rasterizer.h).
 */
#ifndef HSR_FRAME_INGEST_H_INCLUDED
#define HSR_FRAME_INGEST_H_INCLUDED

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSR_INGEST_MAX_LEVELS 3

#define HSR_INGEST_DEPTH_U16 0
#define HSR_INGEST_DEPTH_I32 1
#define HSR_INGEST_DEPTH_F32 2

/* one output level: color [3,H,W] planar fp32, depth [H,W] fp32 */
typedef struct hsr_ingest_level {
    int H, W;
    float* color;
    float* depth;
} hsr_ingest_level;

/* color_u8: [Hs,Ws,3] uint8; depth_raw: [Hs,Ws] of depth_type; labels: [Hs,Ws] int32 or NULL; tree_table: int32 [n_ids,num_levels],
 * NULL when num_levels == 0 (n_ids is then not read); levels: HOST array of n_out entries; out_labels: int64 [num_levels+1,H0,W0] at
 * level 0's size, NULL exactly when labels is NULL (num_levels, tree_table and n_ids are then checked but not used). */
int hsr_frame_ingest(int Hs, int Ws, const uint8_t* color_u8, const void* depth_raw, int depth_type, double depth_scale,
                     const int* labels, int num_levels, const int* tree_table, int n_ids,
                     int n_out, const hsr_ingest_level* levels, int64_t* out_labels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSR_FRAME_INGEST_H_INCLUDED */
