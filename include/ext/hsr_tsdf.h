/*
 * hsr_tsdf.h — C ABI of the mesh of a finished run (libhsr_rast.so), DESIGN.md §7 row 14: rendered depth fused into a truncated signed
 * distance volume, and the volume's zero surface as a triangle mesh.  The reference has NO mesher — its family fuses the rendered depth
 * of the finished map with Open3D's TSDF integration and takes Open3D's mesh — so nothing here is pinned by reference outputs: every
 * rule below is RESTATED here, and tests/tsdf_ref.py restates it once more in numpy for the tests.  An extension under include/ext/: the
 * prototypes under include/hsr_*.h are a counted set (tests/test_abi.py); these are bound under this header's key in
 * diff_gaussian_rasterization/_abi.py HEADERS.
 *
 * All pointers are DEVICE pointers and contiguous, except `w2c`: a HOST array of 16 floats (row-major world-to-camera, rows 0..2 are
 * read) that is copied into the kernel arguments by value.  Everything runs on `stream`; no entry point allocates or synchronises with
 * the host.  Every refusal returns HSR_ERR_INVALID_ARGUMENT (-1) before any device work, with a message in hsr_last_error()
 * (hsr_rasterizer.h) that starts "tsdf_integrate: ", "tsdf_count: ", "tsdf_faces: " or "tsdf_vertices: ".  No kernel here waits for
 * another workgroup and none uses an atomic: every output element has one owner.
 *
 * The volume: an X x Y x Z grid of sample points, x fastest: lin = (k * Y + j) * X + i (64-bit in the kernels).  Point (i, j, k) lies at
 *   px = ox + h * (float)i,  py = oy + h * (float)j,  pz = oz + h * (float)k      one multiply, one add, float32; h is the voxel size.
 * The state, owned by the caller (type, initial value):
 *   tsdf f32 [Z,Y,X] 1   weight f32 [Z,Y,X] 0   color f32 [3,Z,Y,X] 0   cweight f32 [Z,Y,X] 0   best f32 [Z,Y,X] +inf   label i32 [Z,Y,X] -1
 * color / cweight and best / label are optional, NULL in pairs.
 * Refused by every entry point: a side < 1, X * Y * Z > 2^31 - 1.
 *
 * hsr_tsdf_integrate — one view into the volume, ONE launch.  Per sample point, in float32, every operation rounded once, in exactly
 * this order (the file is built without contraction; the numpy restatement matches bit for bit):
 *   xc = ((m00 * px + m01 * py) + m02 * pz) + m03, likewise yc (row 1) and zc (row 2);            skip unless zc > 0
 *   u = fx * (xc / zc) + cx,  v = fy * (yc / zc) + cy;  fu = floorf(u + 0.5f),  fv = floorf(v + 0.5f)
 *   skip unless 0 <= fu < W and 0 <= fv < H, tested in float BEFORE the conversion (a NaN or a huge value skips); pix = (int)fv * W + (int)fu
 *   d = depth[pix];                                                                               skip unless d > 0 and d is finite
 *   depth_max > 0: skip when d > depth_max;   opacity given: skip unless opacity[pix] > sil_thres
 *   sdf = d - zc;  skip when sdf < -trunc;  t = fminf(1, sdf / trunc)
 *   w = weight:  tsdf = (tsdf * w + t) / (w + 1),  weight = fminf(w + 1, max_weight)
 *   image given (planar float [3,H,W]) and fabsf(sdf) <= trunc, with cw = cweight:
 *       color[c] = (color[c] * cw + image[c][pix]) / (cw + 1) for c = 0, 1, 2,  cweight = fminf(cw + 1, max_weight)
 *   labels given (int64 [H,W]) and fabsf(sdf) <= trunc and fabsf(sdf) < best:   best = fabsf(sdf),  label = (int32)labels[pix]
 * A lane owns four consecutive lin (consecutive x) and moves them as 16-byte pieces; the state is read only where one of the four is
 * updated and written only there.  A one-point variant with equal results takes every call whose X * Y * Z is no multiple of 4 or whose
 * state pointers are not 16-byte aligned.
 * Refused: h, trunc or max_weight not finite and positive; H or W outside 1..HSR_TSDF_MAX_IMAGE_SIDE; a NULL w2c, depth, tsdf or weight;
 * color without cweight or the reverse, best without label or the reverse; image without color / cweight, labels without best / label.
 *
 * The surface: marching tetrahedra on the Kuhn decomposition of every cube — no case table, and neighbouring cubes agree on the
 * diagonal of the face they share.
 *   cube      the eight points (i..i+1, j..j+1, k..k+1), named by lin of (i, j, k); meshed only when all eight weights are > 0
 *   inside    tsdf < 0 (an exact 0 is outside)
 *   corners   numbered dx + 2 * dy + 4 * dz
 *   tetrahedra  six per cube, one per axis order (x,y,z), (x,z,y), (y,x,z), (y,z,x), (z,x,y), (z,y,x): for (a,b,c) v0 = corner 0,
 *             v1 = v0 + e_a, v2 = v1 + e_b, v3 = v2 + e_c = corner 7.  Its orientation det[v1 - v0, v2 - v0, v3 - v0] is the parity of the
 *             order: +, -, -, +, +, -
 *   edge key  a mesh vertex lives on a grid edge from a point to that point plus an offset in {0,1}^3 and is named by the int64
 *             lin(lower endpoint) * 8 + (dx + 2 * dy + 4 * dz)
 *   1 or 3 inside   one triangle on the three edges at the lone vertex p, towards the other three in their order within the tetrahedron
 *   2 inside  a < b inside, c < d outside (positions within the tetrahedron): the quad ac, ad, bd, bc, split into two triangles along
 *             the diagonal through the quad vertex with the smallest edge key: (q_m, q_m+1, q_m+2) and (q_m, q_m+2, q_m+3), cyclic
 *   orientation  every triangle's normal points from inside to outside.  With s the tetrahedron's orientation: the lone vertex at
 *             position m keeps the listed order when it is inside and s * (-1)^m > 0, or outside and s * (-1)^m < 0, else the last two
 *             vertices swap; the quad keeps the listed order when s * (-1)^n > 0, n the number of pairs (inside position > outside
 *             position), else it is bc, bd, ad, ac.  (det[q1 - p, q2 - p, q3 - p] > 0 makes the triangle pq1, pq2, pq3 face away from p.)
 *   order     cubes in linear order, tetrahedra in the order above: two runs give identical bytes.
 *
 * hsr_tsdf_count    out_counts[lin] = triangles of cube lin, int32, all X * Y * Z entries written (0 for the last layer of each axis).
 * hsr_tsdf_faces    out_keys [T,3] int64: the triangles' edge keys.  `offsets` [X*Y*Z] int64 is the INCLUSIVE running sum of out_counts
 *                   (torch.cumsum); cube lin writes rows offsets[lin] - count .. offsets[lin] - 1, and nothing where that would pass T.
 *                   T == 0 launches nothing.
 * hsr_tsdf_vertices V edge keys (the sorted unique ones) into positions, colours and labels.  s0, s1: tsdf at the lower and the upper
 *                   endpoint, p0, p1 their positions by the expression above:
 *     t = s0 / (s0 - s1),  out_vertices[v][c] = p0[c] + t * (p1[c] - p0[c])                         float32 [V,3]
 *     out_rgb     uint8 [V,3], per channel: c0 + t * (c1 - c0) when both endpoints have cweight > 0, the one that has it when one
 *                 does, 0.5f when neither; then (uint8)rintf(clamp(c, 0, 1) * 255), as hsr_frame_export rounds (a NaN gives 0)
 *     out_labels  int32 [V]: the label of the endpoint with the smaller fabsf(tsdf), the lower one on a tie
 *   A key whose endpoints are not both grid points writes nothing.  out_rgb needs color and cweight, out_labels needs label; either
 *   output may be NULL.  V == 0 launches nothing.  Refused: h not finite and positive, a NULL keys, tsdf or out_vertices with V > 0,
 *   V > 2^31 - 1.
 */
#ifndef HSR_TSDF_H_INCLUDED
#define HSR_TSDF_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#define HSR_TSDF_MAX_IMAGE_SIDE 16384

#ifdef __cplusplus
extern "C" {
#endif

int hsr_tsdf_integrate(int X, int Y, int Z, float ox, float oy, float oz, float h, float trunc, float max_weight,
                       int H, int W, float fx, float fy, float cx, float cy, const float* w2c,
                       const float* depth, const float* image, const int64_t* labels, const float* opacity, float sil_thres, float depth_max,
                       float* tsdf, float* weight, float* color, float* cweight, float* best, int* label, void* stream);

int hsr_tsdf_count(int X, int Y, int Z, const float* tsdf, const float* weight, int* out_counts, void* stream);

int hsr_tsdf_faces(int X, int Y, int Z, const float* tsdf, const float* weight, const int64_t* offsets, size_t T, int64_t* out_keys,
                   void* stream);

int hsr_tsdf_vertices(int X, int Y, int Z, float ox, float oy, float oz, float h, size_t V, const int64_t* keys,
                      const float* tsdf, const float* color, const float* cweight, const int* label,
                      float* out_vertices, uint8_t* out_rgb, int* out_labels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSR_TSDF_H_INCLUDED */
