// hsr_ingest_expr.h — what the sensor ingest and the units around it state ONCE (internal, not part of the C ABI).  The two value
// expressions: hsr_frame_ingest.hip writes its outputs with them and hsr_keyframe_pack.hip inverts and re-applies them, so "a packed
// keyframe unpacks to the ingest's own bits" holds by construction.  The bilinear taps along one axis, in the real type of the caller
// (hsr_frame_ingest.hip double, hsr_frame_resample.hip float), and the host's test of a side.  The device functions are
// __device__ __forceinline__; the including files are compiled with -ffp-contract=off (neither expression has a product next to a sum,
// the flag only keeps the surrounding code as written).
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

// host: a side of a source or destination image that the taps can index
inline bool hsr_side_ok(int v) { return v >= 1 && v <= HSR_RESAMPLE_MAX_SIDE; }
