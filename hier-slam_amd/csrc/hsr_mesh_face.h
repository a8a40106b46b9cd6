// hsr_mesh_face.h — the ONE statement of a mesh face as a view sees it (include/recon/hsr_mesh_depth.h, "The face" and "The box"): its
// camera-space corners by hsr_project.h, the three crosses and det, the clauses by which it takes no part, and its box.  Used by
// hsr_mesh_depth.hip, which decides the face under every pixel with it, and by hsr_mesh_shade.hip, which recomputes that face's terms
// for the pixel's barycentric weights: the same device functions, so the same bits.  Both files are built without contraction: every
// operation is rounded once, in this order.
#pragma once
#include <math.h>

#include <hip/hip_runtime.h>

#include "hsr_project.h"

namespace {      // internal linkage: each of the two files has its own copy

struct View {
    float m[12];      // rows 0..2 of the world-to-camera matrix
    float fx, fy, cx, cy, near;
    int H, W;
};

struct Face {
    float nA[3], nB[3], nC[3], det;
    int x0, x1, y0, y1;      // the box, inclusive
};

__device__ __forceinline__ void cross(const float* P, const float* Q, float* out)
{
    out[0] = P[1] * Q[2] - P[2] * Q[1];
    out[1] = P[2] * Q[0] - P[0] * Q[2];
    out[2] = P[0] * Q[1] - P[1] * Q[0];
}

__device__ __forceinline__ bool finite3(const float* p) { return fabsf(p[0]) < INFINITY && fabsf(p[1]) < INFINITY && fabsf(p[2]) < INFINITY; }

// the clauses of the face f that do not depend on near or on the image: its indices (idx) and camera-space corners A, B, C, the three
// crosses and det; false when an index is outside 0..V-1 or one of them is not finite or det is 0
__device__ __forceinline__ bool face_terms(const float* m, int V, const float* __restrict__ vertices, const int* __restrict__ faces, int f, int* idx,
                                           float* A, float* B, float* C, Face& out)
{
    const int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
    if (!((unsigned)ia < (unsigned)V && (unsigned)ib < (unsigned)V && (unsigned)ic < (unsigned)V)) return false;
    idx[0] = ia; idx[1] = ib; idx[2] = ic;
    const float* a = vertices + 3 * (size_t)ia;
    const float* b = vertices + 3 * (size_t)ib;
    const float* d = vertices + 3 * (size_t)ic;
    hsr_camera_point(m, a[0], a[1], a[2], A[0], A[1], A[2]);
    hsr_camera_point(m, b[0], b[1], b[2], B[0], B[1], B[2]);
    hsr_camera_point(m, d[0], d[1], d[2], C[0], C[1], C[2]);
    if (!(finite3(A) && finite3(B) && finite3(C))) return false;
    cross(B, C, out.nA);
    cross(C, A, out.nB);
    cross(A, B, out.nC);
    if (!(finite3(out.nA) && finite3(out.nB) && finite3(out.nC))) return false;
    out.det = (A[0] * out.nA[0] + A[1] * out.nA[1]) + A[2] * out.nA[2];
    if (!(fabsf(out.det) < INFINITY) || out.det == 0.f) return false;
    return true;
}

// the face f of the header: false when it takes no part or its box is empty
__device__ __forceinline__ bool make_face(const View& c, int V, const float* __restrict__ vertices, const int* __restrict__ faces, int f, Face& out)
{
    int idx[3];
    float A[3], B[3], C[3];
    if (!face_terms(c.m, V, vertices, faces, f, idx, A, B, C, out)) return false;
    if (A[2] < c.near && B[2] < c.near && C[2] < c.near) return false;      // wholly nearer than near, or behind the camera
    if (A[2] < c.near || B[2] < c.near || C[2] < c.near) {
        out.x0 = 0; out.x1 = c.W - 1; out.y0 = 0; out.y1 = c.H - 1;
        return true;
    }
    const float uA = c.fx * (A[0] / A[2]) + c.cx, uB = c.fx * (B[0] / B[2]) + c.cx, uC = c.fx * (C[0] / C[2]) + c.cx;
    const float vA = c.fy * (A[1] / A[2]) + c.cy, vB = c.fy * (B[1] / B[2]) + c.cy, vC = c.fy * (C[1] / C[2]) + c.cy;
    float x0 = floorf(fminf(fminf(uA, uB), uC)) - 1.f, x1 = ceilf(fmaxf(fmaxf(uA, uB), uC)) + 1.f;
    float y0 = floorf(fminf(fminf(vA, vB), vC)) - 1.f, y1 = ceilf(fmaxf(fmaxf(vA, vB), vC)) + 1.f;
    const float xe = (float)(c.W - 1), ye = (float)(c.H - 1);
    if (!(x1 >= 0.f && x0 <= xe && y1 >= 0.f && y0 <= ye)) return false;      // empty (u and v are never NaN: see the header)
    x0 = fmaxf(x0, 0.f); x1 = fminf(x1, xe);
    y0 = fmaxf(y0, 0.f); y1 = fminf(y1, ye);                                  // in float: an infinite bound never reaches (int)
    out.x0 = (int)x0; out.x1 = (int)x1; out.y0 = (int)y0; out.y1 = (int)y1;
    return true;
}

}  // namespace
