// hsr_project.h — the ONE statement of the projection of a world point into a view that decides a pixel (include/ext/hsr_tsdf.h,
// hsr_tsdf_integrate): used by hsr_tsdf.hip for a sample point and by hsr_mesh_eval.hip for a mesh vertex, so that a vertex is seen in
// exactly the pixel a sample point at its place would be fused from.  Both files are built without contraction: every operation is
// rounded once, in this order.
#pragma once
#include <hip/hip_runtime.h>

// m: rows 0..2 of the world-to-camera matrix; the camera-space point of a world point.  The three lines every user of this header
// shares: hsr_project_pixel below, and hsr_mesh_depth.hip for the corners of a face.
__device__ __forceinline__ void hsr_camera_point(const float* m, float px, float py, float pz, float& xc, float& yc, float& zc)
{
    xc = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3];
    yc = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7];
    zc = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11];
}

// m: rows 0..2 of the world-to-camera matrix.  False unless zc > 0 and the pixel centre nearest to the projection lies in the H x W
// image; then zc is the depth along the camera's axis and pix = row * W + column.
__device__ __forceinline__ bool hsr_project_pixel(const float* m, float fx, float fy, float cx, float cy, int H, int W, float px, float py,
                                                  float pz, float& zc, int& pix)
{
    float xc, yc;
    hsr_camera_point(m, px, py, pz, xc, yc, zc);
    if (!(zc > 0.f)) return false;
    const float u = fx * (xc / zc) + cx, v = fy * (yc / zc) + cy;
    const float fu = floorf(u + 0.5f), fv = floorf(v + 0.5f);
    if (!(fu >= 0.f && fu < (float)W && fv >= 0.f && fv < (float)H)) return false;      // in float: a NaN or 1e30 never reaches (int)
    pix = (int)fv * W + (int)fu;                                                          // < 2^28: both sides <= 16384
    return true;
}
