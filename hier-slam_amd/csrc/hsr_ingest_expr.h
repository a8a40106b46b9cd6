// hsr_ingest_expr.h — what the sensor ingest and the units around it state ONCE (internal, not part of the C ABI).  The two value
// expressions: hsr_frame_ingest.hip writes its outputs with them and hsr_keyframe_pack.hip inverts and re-applies them, so "a packed
// keyframe unpacks to the ingest's own bits" holds by construction.  The bilinear taps along one axis, in the real type of the caller
// (hsr_frame_ingest.hip double, hsr_frame_resample.hip float), and the host's test of a side.  The source coordinates of an undistorted
// pixel and their quantisation (include/sensor/hsr_frame_undistort.h; hsr_frame_ingest.hip).  The device functions are
// __device__ __forceinline__; the including files are compiled with -ffp-contract=off (neither value expression has a product next to a
// sum, there the flag only keeps the surrounding code as written; the coordinate expressions do, and need it).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ext/hsr_frame_resample.h"

// include/ext/hsr_frame_ingest.h, COLOUR: float(v) / 255.0f for a value v already rounded to fp32 — through double: the double quotient
// of two floats rounds to the correctly rounded fp32 quotient
__device__ __forceinline__ float hsr_ingest_colour(float v) { return (float)((double)v / 255.0); }

// include/ext/hsr_frame_ingest.h, DEPTH: float(double(raw) / depth_scale)
__device__ __forceinline__ float hsr_ingest_depth(double raw, double depth_scale) { return (float)(raw / depth_scale); }

// the left tap, the right one and the weight of the right one along one axis: destination index i of nd from ns source samples
// (include/ext/hsr_frame_resample.h, COLOUR)
template <typename Real>
__device__ __forceinline__ void hsr_taps(int i, int ns, int nd, int& i0, int& i1, Real& f)
{
    int n = (2 * i + 1) * ns - nd;      // <= (2 * 16383 + 1) * 16384 < 2^30
    n = n > 0 ? n : 0;
    i0 = n / (2 * nd);
    f = (Real)(n - i0 * 2 * nd) / (Real)(2 * nd);
    i1 = i0 + 1 < ns ? i0 + 1 : ns - 1;
}

// the camera of the sensor image and its five Brown-Conrady coefficients, OpenCV's order (include/sensor/hsr_frame_undistort.h)
struct hsr_lens {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;
};

// include/sensor/hsr_frame_undistort.h, U, the source coordinates (us, vs) of the undistorted pixel (u, v): in double, one rounding per
// operation, in the header's association (the including file is compiled with -ffp-contract=off: here products DO stand next to sums)
__device__ __forceinline__ void hsr_undistort_source(int u, int v, const hsr_lens& m, double& us, double& vs)
{
    const double x = ((double)u - m.cx) / m.fx, y = ((double)v - m.cy) / m.fy;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2.0 * (x * y);
    const double kr = 1.0 + ((m.k3 * r2 + m.k2) * r2 + m.k1) * r2;
    const double xd = x * kr + m.p1 * xy2 + m.p2 * (r2 + 2.0 * x2);
    const double yd = y * kr + m.p1 * (r2 + 2.0 * y2) + m.p2 * xy2;
    us = m.fx * xd + m.cx;
    vs = m.fy * yd + m.cy;
}

// the same header, the quantisation of one coordinate to 1/32 pixel: the tap s = floor(i / 32) and the weight a = i - 32 * s of the tap
// after it, i = rint(clamp(32 * c, -2^30, 2^30)) half to even; false for a NaN (s and a are then not set)
__device__ __forceinline__ bool hsr_undistort_step(double c, int& s, int& a)
{
    const double q = c * 32.0;
    if (q != q) return false;
    const int i = (int)rint(fmin(fmax(q, -1073741824.0), 1073741824.0));      // |i| <= 2^30
    s = i >> 5;      // arithmetic: floor division
    a = i & 31;
    return true;
}

// host: a side of a source or destination image that the taps can index
inline bool hsr_side_ok(int v) { return v >= 1 && v <= HSR_RESAMPLE_MAX_SIDE; }
