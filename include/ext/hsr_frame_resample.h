/*
 * hsr_frame_resample.h — C ABI of the device resample of one RGB-D frame (libhsr_rast.so), DESIGN.md §7 row 8: the frames the
 * reference's second and third dataset objects deliver when tracking or densification run at a resolution of their own
 * (scripts/hierslam.py:1543-1563, :1680-1699, :1792-1799, :1933-1941; datasets/gradslam_datasets/basedataset.py:223-227 for the colour
 * image, :248-252 for the depth map).  An extension under include/ext/: the prototypes under include/hsr_*.h are a counted set
 * (tests/test_abi.py); this one is bound under its key in diff_gaussian_rasterization/_abi.py HEADERS.
 *
 * RESTATED, NOT PINNED BY cv2: the reference resizes with cv2.resize, which is not available to this project's tests.  Both rules
 * are restated below and checked against two independent float64 restatements (tests/resample_ref.py: torch F.interpolate, and
 * scipy.ndimage.map_coordinates / integer indexing).  The reference resizes the colour image before the / 255 of scripts/hierslam.py,
 * but not as uint8: it reads the image with dtype=float (basedataset.py:298, replica.py:381), so cv2 interpolates in float64 on the
 * values 0..255 and rounds to no grey level.  This kernel interpolates the fp32 image in 0..1 with fp32 weights and rounds nothing
 * either, so its colours differ from the reference's only by fp32 rounding (about 5e-7 of the 0..1 range) — and, when the frame it is
 * given was itself quantised or resized, by that.  hsr_frame_ingest.h interpolates the 8-bit sensor image in float64 as the reference
 * does and is the closer of the two.  The depth rule copies and has no such difference.
 *
 * One call is ONE launch and produces up to two levels (H0,W0) and (H1,W1) of the same source frame; H1 == 0 skips level 1 (its
 * two pointers are then not read and nothing is written through them).  Source and destination sides are each 1 .. HSR_RESAMPLE_MAX_SIDE,
 * a destination smaller or larger than the source; anything else returns HSR_ERR_INVALID_ARGUMENT and launches nothing.
 *
 * COLOUR — bilinear, as cv2.resize(..., interpolation=INTER_LINEAR): half-pixel centres, replicated border, no antialiasing.
 * For destination column x of a row of Wd columns resampled from W columns, in integers:
 *     n  = max((2x + 1) * W - Wd, 0)          twice-Wd times the source coordinate (x + 0.5) * W / Wd - 0.5, clamped at 0
 *     x0 = n / (2 * Wd)                        integer division: the left tap
 *     fx = float(n - x0 * 2 * Wd) / float(2 * Wd)      both operands are integers of at most 2^15: exact in fp32, one rounding
 *     x1 = min(x0 + 1, W - 1)                  the right tap, clamped (x0 <= W - 1 always)
 * and the same for destination row y with H, Hd: y0, fy, y1.  With a = src[y0][x0], b = src[y0][x1], c = src[y1][x0], d = src[y1][x1]
 * of one channel, in fp32 and in this order, without fused multiply-add (the file is compiled with -ffp-contract=off):
 *     top = a + fx * (b - a),   bot = c + fx * (d - c),   value = top + fy * (bot - top).
 * The sample positions are exact because they are integers.  Equal sizes give fx = fy = 0, hence a copy: bit-exact for finite
 * input whose differences are finite (a negative zero comes out as +0).
 *
 * DEPTH — nearest, as cv2.resize(..., interpolation=INTER_NEAREST): the source index is
 *     xs = (x * W) / Wd,   ys = (y * H) / Hd          integer division (never beyond W - 1, H - 1)
 * and the 32 bits of src[ys][xs] are copied: zeros (holes), NaN and inf travel unchanged.  This equals cv2's documented
 * floor(x * (1 / (Wd / W))) in double and torch's mode='nearest' at every index of the size pairs of tests/test_gpu_frame_resample.py.
 *
 * All pointers are DEVICE pointers; maps are planar CHW / HW, fp32, contiguous.  Everything runs on `stream`; nothing synchronises
 * with the host.  Errors: return <0 and hsr_last_error() (hsr_rasterizer.h).  No allocation inside the library, no scratch.
 */
#ifndef HSR_FRAME_RESAMPLE_H_INCLUDED
#define HSR_FRAME_RESAMPLE_H_INCLUDED

#ifdef __cplusplus
extern "C" {
#endif

#define HSR_RESAMPLE_MAX_SIDE 16384

/* color: [3,H,W]; depth: [H,W].  out_color0 [3,H0,W0], out_depth0 [H0,W0]; out_color1 [3,H1,W1], out_depth1 [H1,W1] unless H1 == 0
 * (W1 is then ignored).  No output may overlap an input. */
int hsr_frame_resample(int H, int W, const float* color, const float* depth, int H0, int W0, float* out_color0, float* out_depth0,
                       int H1, int W1, float* out_color1, float* out_depth1, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSR_FRAME_RESAMPLE_H_INCLUDED */
