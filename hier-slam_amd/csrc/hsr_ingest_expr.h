// hsr_ingest_expr.h — the two value expressions of the sensor ingest (internal, not part of the C ABI), stated ONCE: hsr_frame_ingest.hip
// writes its outputs with them and hsr_keyframe_pack.hip inverts and re-applies them, so "a packed keyframe unpacks to the ingest's own
// bits" holds by construction.  Both are __device__ __forceinline__; the including files are compiled with -ffp-contract=off (neither
// expression has a product next to a sum, the flag only keeps the surrounding code as written).
#pragma once
#include <hip/hip_runtime.h>

// include/ext/hsr_frame_ingest.h, COLOUR: float(v) / 255.0f for a value v already rounded to fp32 — through double: the double quotient
// of two floats rounds to the correctly rounded fp32 quotient
__device__ __forceinline__ float hsr_ingest_colour(float v) { return (float)((double)v / 255.0); }

// include/ext/hsr_frame_ingest.h, DEPTH: float(double(raw) / depth_scale)
__device__ __forceinline__ float hsr_ingest_depth(double raw, double depth_scale) { return (float)(raw / depth_scale); }
