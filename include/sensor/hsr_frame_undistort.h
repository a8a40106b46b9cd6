/*
 * hsr_frame_undistort.h — C ABI of the device ingest of one raw sensor frame whose COLOUR image is undistorted on the way
 * (libhsr_rast.so), DESIGN.md §7 row 8.  The reference's dataset objects undistort the colour image, and only it, between the decoded
 * image and the frame loop (datasets/gradslam_datasets/basedataset.py:306-309: cv2.undistort(color, K, self.distortion), "only applied
 * on color image, not depth!"); its TUM RGB-D loader (datasets/gradslam_datasets/tum.py) is the one of this family whose calibrations
 * carry the five Brown-Conrady coefficients.  This entry is hsr_frame_ingest (include/ext/hsr_frame_ingest.h) with that step inside the
 * same single launch: the same kernel runs behind both, with a compile-time flag that says where a colour tap comes from.  It reuses
 * hsr_ingest_level, HSR_INGEST_DEPTH_* and HSR_INGEST_MAX_LEVELS of hsr_frame_ingest.h.  The directory include/sensor/ is its own
 * because the header sets under include/hsr_*.h, include/ext/, include/eval/ and include/recon/ are counted sets (tests/test_abi.py,
 * tests/test_mesh_eval_cpu.py, tests/test_mesh_depth_cpu.py); this one is bound under its key in
 * diff_gaussian_rasterization/_abi.py SENSOR_HEADERS.
 *
 * One call is ONE launch: the arguments, the checks and the outputs are those of hsr_frame_ingest — an 8-bit interleaved colour image,
 * a raw depth image and, optionally, a raw class-id image, all at the sensor size Hs x Ws, become n_out (1 .. HSR_INGEST_MAX_LEVELS)
 * levels of float32 planar colour in 0..1 and float32 depth in metres, plus, at level 0's size only, the int64 label planes.  No
 * scratch, no allocation, no host synchronisation.
 *
 * HSR_ERR_INVALID_ARGUMENT, and nothing launched, for:
 *   - everything hsr_frame_ingest refuses (its header lists it), the message beginning "frame_ingest_undistort:";
 *   - fx or fy zero or not finite;
 *   - any of cx, cy, k1, k2, p1, p2, k3 not finite.
 * No output may overlap an input.
 *
 * DEPTH, LABELS — NOT undistorted, as in the reference: the nearest rules of hsr_frame_ingest.h, unchanged, bit for bit.
 *
 * COLOUR — the bilinear rule of hsr_frame_ingest.h applied to the undistorted sensor image U (defined below): with the taps x0, x1, fx_w
 * and y0, y1, fy_w of that header, a = U[y0][x0][ch], b = U[y0][x1][ch], c = U[y1][x0][ch], d = U[y1][x1][ch] are VALUES OF U, not 8-bit
 * pixels, and in float64, in this order, without fused multiply-add (the file is compiled with -ffp-contract=off):
 *     top = a + fx_w * (b - a),   bot = c + fx_w * (d - c),   v = top + fy_w * (bot - top)
 * The output is float(v) / 255.0f.  A level of the sensor's size has weights 0, so it is U itself: a + 0 * (b - a) is a bit for bit,
 * and the kernel evaluates one tap there.
 *
 * U — U[v][u][ch] for the integer sensor pixel (u, v).  The source coordinates, in float64, one rounding per operation, in exactly
 * this association (fx, fy, cx, cy are those of the SENSOR image, in its pixels; k1, k2, p1, p2, k3 in OpenCV's order):
 *     x = (u - cx) / fx          y = (v - cy) / fy
 *     x2 = x*x    y2 = y*y    r2 = x2 + y2    xy2 = 2.0 * (x*y)
 *     kr = 1.0 + ((k3*r2 + k2)*r2 + k1)*r2
 *     xd = x*kr + p1*xy2 + p2*(r2 + 2.0*x2)
 *     yd = y*kr + p1*(r2 + 2.0*y2) + p2*xy2
 *     us = fx*xd + cx            vs = fy*yd + cy
 * (sums of three terms from the left).  Quantisation to 1/32 pixel:
 *     iu = rint(clamp(us * 32.0, -2^30, 2^30))      rounded half to even; the same for iv from vs
 *     a NaN us * 32.0 or vs * 32.0 makes U[v][u] 0 in all channels
 *     sx = floor(iu / 32),  ax = iu - 32 * sx       floor division (sx = iu >> 5, ax = iu & 31 in two's complement), so negative
 *                                                   coordinates work; the same for sy, ay
 * The four taps are (sy,sx), (sy,sx+1), (sy+1,sx), (sy+1,sx+1) of the 8-bit image; a tap outside the image is 0.  With their values
 * a, b, c, d
 *     U = (a*(32-ax)*(32-ay) + b*ax*(32-ay) + c*(32-ax)*ay + d*ax*ay) / 1024
 * The numerator is an integer below 2^18, so U is exact in float64 (and in fp32) in any order of evaluation: only the coordinates
 * carry rounding.
 *
 * RESTATED, NOT PINNED BY cv2: the reference undistorts with cv2.undistort, which is not available to this project's tests.  The rule
 * above is cv2.undistort(color, K, dist) with newCameraMatrix = K as believed from OpenCV's sources and NOT CHECKED here: coordinates
 * kept to 1/32 pixel (INTER_BITS = 5), INTER_LINEAR weights that are the exact products of those fractions, BORDER_CONSTANT 0, and a
 * float64 image (basedataset.py:298 reads with dtype=float) that is rounded to no grey level.  One known difference: cv2 builds its
 * coordinate map incrementally, in stripes, through an inverted matrix, so its coordinates differ from the ones above in the last
 * bits, and a pixel whose us * 32 (or vs * 32) lies that close to a half-integer may take the neighbouring 1/32 step.  No more is
 * claimed.
 *
 * SIZE: the reference resizes first and then undistorts with the UNSCALED K, which is correct geometry only when the frame has the
 * sensor's size — every TUM configuration of this family (480x640, nothing reduced).  Here a reduced level is the resize of the
 * correctly undistorted sensor image.  At the sensor's size the two orders are the same thing; at a reduced size this is a stated
 * difference, not a defect to reproduce.
 *
 * ZERO DISTORTION: with the five coefficients zero us is within 3e-14 of u (480x640 with TUM fr3's intrinsics), iu = 32 * u, and the
 * output equals hsr_frame_ingest's bit for bit.
 *
 * All pointers are DEVICE pointers except `levels`, a HOST array whose structs are copied into the kernel's arguments by value.
 * Everything runs on `stream`.  Errors: return <0 and hsr_last_error() (hsr_rasterizer.h).
 */
#ifndef HSR_FRAME_UNDISTORT_H_INCLUDED
#define HSR_FRAME_UNDISTORT_H_INCLUDED

#include <stdint.h>

#include "../ext/hsr_frame_ingest.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the arguments of hsr_frame_ingest, and between n_ids and n_out the camera of the SENSOR image and its five coefficients */
int hsr_frame_ingest_undistort(int Hs, int Ws, const uint8_t* color_u8, const void* depth_raw, int depth_type, double depth_scale,
                               const int* labels, int num_levels, const int* tree_table, int n_ids,
                               double fx, double fy, double cx, double cy,
                               double k1, double k2, double p1, double p2, double k3,
                               int n_out, const hsr_ingest_level* levels, int64_t* out_labels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSR_FRAME_UNDISTORT_H_INCLUDED */
