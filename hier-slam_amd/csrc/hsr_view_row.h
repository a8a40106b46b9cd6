// hsr_view_row.h — the per-Gaussian arithmetic of include/ext/hsr_view.h, stated once (internal, not part of the C ABI): input row `src`
// of the map to output row `dst` of the rasterizer's arrays.  hsr_view.hip runs it with dst == src over the whole map, hsr_replay.hip
// with dst = the rank of a selected row.  __device__ __forceinline__, so the including file's flags apply (both are compiled with
// -ffp-contract=off: out_means3D feeds the rasterizer's integer decisions).
#pragma once
#include "hsr_quat.h"
#include "../../include/hsr_frame_prep.h"

struct ViewArgs {
    int P, S, transform_rots, rot_source;
    const float *means3D, *unnorm_rotations, *logit_opacities, *log_scales, *w2c;
};

// F.normalize(matrix_to_quaternion(w2c[:3,:3])): hsr_utils/slam.py matrix_to_quaternion, then eval_helpers.py:1708
__device__ __forceinline__ void view_quaternion(const float* __restrict__ m, float* q)
{
    const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[4], m11 = m[5], m12 = m[6], m20 = m[8], m21 = m[9], m22 = m[10];
    const float p0 = ((1.0f + m00) + m11) + m22, p1 = ((1.0f + m00) - m11) - m22;
    const float p2 = ((1.0f - m00) + m11) - m22, p3 = ((1.0f - m00) - m11) + m22;
    // argmax: the largest pivot, the first on ties
    float pv = p0;
    float4 r = make_float4(p0, m21 - m12, m02 - m20, m10 - m01);
    if (p1 > pv) { pv = p1; r = make_float4(m21 - m12, p1, m10 + m01, m02 + m20); }
    if (p2 > pv) { pv = p2; r = make_float4(m02 - m20, m10 + m01, p2, m21 + m12); }
    if (p3 > pv) { pv = p3; r = make_float4(m10 - m01, m02 + m20, m21 + m12, p3); }
    const float d = 2.0f * sqrtf(fmaxf(pv, 1e-12f));
    r = make_float4(r.x / d, r.y / d, r.z / d, r.w / d);
    if (r.x < 0.0f) r = make_float4(-r.x, -r.y, -r.z, -r.w);
    r = hsr_normalize4(r);
    q[0] = r.x; q[1] = r.y; q[2] = r.z; q[3] = r.w;
}

// WORLD: the means stay in the world frame (a bit copy; a.w2c is not read for them)
template <bool WORLD>
__device__ __forceinline__ void view_row(const ViewArgs& a, size_t src, size_t dst, float* __restrict__ out_means3D,
                                         float* __restrict__ out_unnorm_rot, float* __restrict__ out_rotations,
                                         float* __restrict__ out_opacities, float* __restrict__ out_scales)
{
    const float x0 = a.means3D[3 * src], x1 = a.means3D[3 * src + 1], x2 = a.means3D[3 * src + 2];
    if (WORLD) {
        out_means3D[3 * dst] = x0; out_means3D[3 * dst + 1] = x1; out_means3D[3 * dst + 2] = x2;
    } else {
#pragma unroll
        for (int i = 0; i < 3; i++)
            out_means3D[3 * dst + i] = ((x0 * a.w2c[4 * i] + x1 * a.w2c[4 * i + 1]) + x2 * a.w2c[4 * i + 2]) + a.w2c[4 * i + 3];
    }
    const float4 u = reinterpret_cast<const float4*>(a.unnorm_rotations)[src];
    float4 tr = u;
    if (a.transform_rots) {
        float q[4];
        view_quaternion(a.w2c, q);
        tr = hsr_quat_mult(q, hsr_normalize4(u));
    }
    if (out_unnorm_rot) reinterpret_cast<float4*>(out_unnorm_rot)[dst] = tr;
    reinterpret_cast<float4*>(out_rotations)[dst] = hsr_normalize4(a.rot_source == HSR_PREP_ROT_PARAMS ? u : tr);
    out_opacities[dst] = 1.0f / (1.0f + expf(-a.logit_opacities[src]));
    if (a.S == 1) {
        const float e = expf(a.log_scales[src]);
        out_scales[3 * dst] = e; out_scales[3 * dst + 1] = e; out_scales[3 * dst + 2] = e;
    } else {
#pragma unroll
        for (int i = 0; i < 3; i++) out_scales[3 * dst + i] = expf(a.log_scales[3 * src + i]);
    }
}
