// hsr_quat.h — the quaternion expressions of the rasterizer-input preparation (internal, not part of the C ABI), shared by
// hsr_frame_prep.hip (a pose column) and hsr_view.hip (a given matrix) so that equal inputs give equal bits in both.  Every function is
// __device__ __forceinline__: the including file's flags (-ffp-contract=off, csrc/Makefile) apply to the inlined code.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float4 hsr_quat_mult(const float* a, float4 b)  // slam_helpers.py:21-28, a = q1, b = q2 (w, x, y, z)
{
    float4 o;
    o.x = ((a[0] * b.x - a[1] * b.y) - a[2] * b.z) - a[3] * b.w;
    o.y = ((a[0] * b.y + a[1] * b.x) + a[2] * b.w) - a[3] * b.z;
    o.z = ((a[0] * b.z - a[1] * b.w) + a[2] * b.x) + a[3] * b.y;
    o.w = ((a[0] * b.w + a[1] * b.z) - a[2] * b.y) + a[3] * b.x;
    return o;
}

__device__ __forceinline__ float hsr_norm4(float4 v) { return sqrtf(((v.x * v.x + v.y * v.y) + v.z * v.z) + v.w * v.w); }

// F.normalize: v / max(|v|, 1e-12)
__device__ __forceinline__ float4 hsr_normalize4(float4 v, float* n_out = nullptr)
{
    const float n = hsr_norm4(v);
    if (n_out) *n_out = n;
    const float d = fmaxf(n, 1e-12f);
    return make_float4(v.x / d, v.y / d, v.z / d, v.w / d);
}
