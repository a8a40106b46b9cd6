/*
 * hsr_mesh_shade.h — C ABI of the pictures of a triangle mesh from a given view (libhsr_rast.so), DESIGN.md §7 row 20: area-weighted
 * vertex normals, and the deferred pass that turns the face image of hsr_mesh_depth (include/recon/hsr_mesh_depth.h) and the mesh's
 * attributes into 8-bit pictures — shaded, in vertex colours, in class colours, normals, a scalar per vertex as a heat map — all
 * pictures of a view in ONE launch (hsr_utils/mesh_view.py).  The reference family leaves the device for Open3D's window here, so
 * nothing is pinned by reference outputs: both rules are RESTATED below, and tests/mesh_view_ref.py restates them once more in numpy.
 * The header lives under include/shade/: the other directories under include/ are counted sets held by their own suites; these
 * prototypes are bound under this header's key in diff_gaussian_rasterization/_abi.py SHADE_HEADERS.
 *
 * All pointers are DEVICE pointers and contiguous, except `w2c` (a HOST array of 16 floats, row-major world-to-camera, rows 0..2 are
 * read) and `jobs` (a HOST array of structs); both are copied into the kernel arguments by value.  Everything runs on `stream`; no
 * entry point allocates or synchronises with the host.  Every refusal returns HSR_ERR_INVALID_ARGUMENT (-1) before any device work,
 * with a message in hsr_last_error() (hsr_rasterizer.h) that starts "mesh_shade: ".  The file is built without contraction and uses no
 * transcendental function: every operation below is rounded once, in exactly the stated order; sqrt and the divisions are the
 * correctly rounded ones.  The numpy restatement matches bit for bit.
 *
 * ---- hsr_mesh_normals ----------------------------------------------------------------------------------------------------------------
 * hsr_mesh_normals_scratch_bytes(V): 24 bytes a vertex (three 64-bit accumulators), rounded up to 16; 0 for a negative V.
 * hsr_mesh_normals: out_normals float32 [V,3], the area-weighted normal of every vertex of the mesh (vertices float32 [V,3], faces
 * int32 [F,3]) in WORLD space.  The sums are integers, so the result does not depend on the order of arrival and is the same bytes on
 * every run.
 *   The face, in float32: A, B, C its corners;  e1 = B - A,  e2 = C - A (per component);  c = cross(e1, e2) with
 *     cross(P, Q) = (Py * Qz - Pz * Qy,  Pz * Qx - Px * Qz,  Px * Qy - Py * Qx)         as in hsr_mesh_depth.h; |c| is twice the area
 *   A face takes NO part when one of its indices is outside 0..V-1, a component of c is not finite, or |component| >= 2^16 (65536).
 *   Per component q = llrint((double)c * 2^40): the product is exact (a power of two), the rounding is to nearest, halves to even;
 *     |q| < 2^56.  q is added to the accumulator of that component at each of the three corners: a 64-bit integer atomic add at agent
 *     scope whose result is not used.  Integer addition is associative and commutative, wrap-around included.
 *   The vertex, second kernel: per component d = (double)s * 2^-40 with s the accumulator as a signed 64-bit integer ((double)s is
 *     rounded to nearest even when |s| >= 2^53);  len = sqrt((dx * dx + dy * dy) + dz * dz) in float64;  n = (float)(d / len) per
 *     component, one float64 division and one rounding to float32;  n = (0, 0, 0) when len == 0.
 * The entry point zeroes the accumulators on the stream first, so a scratch carries nothing from one call to the next; F = 0 writes
 * zeros.  Refused: V < 1; F < 0; a NULL vertices, scratch or out_normals; a NULL faces with F > 0; scratch_bytes below
 * hsr_mesh_normals_scratch_bytes(V); a scratch that is not 16-byte aligned.
 *
 * ---- hsr_mesh_shade ------------------------------------------------------------------------------------------------------------------
 * ONE launch for n_jobs (1 .. HSR_SHADE_MAX_JOBS) pictures of ONE view; each picture is uint8 [H,W,3] with the bytes R, G, B in memory,
 * as in hsr_frame_export.h.  face_image int32 [H,W] is hsr_mesh_depth's out_face for the same mesh, camera and w2c.  What depends on
 * the pixel alone is computed once and shared by all jobs.
 *
 * The pixel (x, y), f = face_image[y * W + x].  It gets the job's BACKGROUND colour, in every job, when f is outside 0..F-1, or the
 * face takes no part by the clauses of hsr_mesh_depth.h that need neither near nor the image (an index outside 0..V-1; a camera-space
 * coordinate, a component of the three crosses or det not finite; det == 0) — these are computed by the device functions the depth
 * kernel uses (csrc/hsr_mesh_face.h), so A, B, C, nA, nB, nC and det are the same bits — or when s or z below fail.  Otherwise:
 *   rx = ((float)x - cx) / fx,  ry = ((float)y - cy) / fy
 *   wA = (rx * nAx + ry * nAy) + nAz,  likewise wB and wC;  s = (wA + wB) + wC                  exactly the hit test's
 *   background when s == 0;   bA = wA / s,  bB = wB / s,  bC = wC / s;   z = det / s;   background unless 0 < z < +inf
 *   (of a face image that hsr_mesh_depth wrote for this mesh and view no pixel fails here: it stored this z, and z >= near > 0).
 * The weights are perspective-correct: the test is ray casting in camera space, so wA / s is the barycentric weight of A at the point
 * where the ray meets the face's plane in 3D, not a weight interpolated in the image plane.
 *   p = (z * rx, z * ry, z)  the hit point;   l = sqrtf((px * px + py * py) + pz * pz);   v = (-px / l, -py / l, -pz / l)
 *
 * The flat normal, shared by all jobs:  e1 = B - A, e2 = C - A in camera space,  g = cross(e1, e2),
 *   gl = sqrtf((gx * gx + gy * gy) + gz * gz);  nf = (gx / gl, gy / gl, gz / gl) when 0 < gl < +inf, else nf = (0, 0, -1).
 * The shading normal of a job:  job.normals == NULL: n = nf.  Otherwise normals is float32 [V,3] in world space, and per corner P
 *   nP' = ((m00 * nPx + m01 * nPy) + m02 * nPz,  (m10 * ..) ..,  (m20 * ..) ..)          the rotation rows of w2c, no translation
 *   t = ((bA * nA'x + bB * nB'x) + bC * nC'x, likewise y and z);   tl = sqrtf((tx * tx + ty * ty) + tz * tz)
 *   n = (tx / tl, ty / tl, tz / tl) when 0 < tl < +inf (a NaN fails), else n = nf.
 * Then, for either:  n is negated when (nx * px + ny * py) + nz * pz > 0 — shading is two-sided, so a winding never blackens a
 * picture — and   shade = ambient + (1.0f - ambient) * fabsf((nx * vx + ny * vy) + nz * vz).
 *
 * The byte of a float colour t, HSR_EXPORT_COLOR's rule:  c = t > 0 ? (t < 1 ? t : 1) : 0 (a NaN gives 0);  byte = c * 255.0f rounded
 * to the nearest integer, halves to even.  Lighting a table colour (r, g, b bytes): lit != 0: byte((float)r / 255.0f * shade), the
 * division first; lit == 0: the table's bytes as they are.
 *
 * SHADED — byte(albedo[k] * shade) for k = R, G, B.  attr, table and lit are not read.
 * COLOUR — attr uint8 [V,3]: per channel t = ((bA * (float)cA + bB * (float)cB) + bC * (float)cC) / 255.0f;  lit != 0: t = t * shade;
 *   byte(t).
 * NORMALS — byte(nx * 0.5f + 0.5f), byte((-ny) * 0.5f + 0.5f), byte((-nz) * 0.5f + 0.5f): a surface that faces the camera is blue.
 * LABELS — attr int32 [V], table uint8 [n,3]: the label of the corner with the largest weight, the lowest slot on ties (k = A; B when
 *   bB > bk; C when bC > bk).  0 <= label < n: table[label], lit as above; else black (0, 0, 0), as HSR_EXPORT_LABELS, lit or not.
 * SCALAR — attr float32 [V], table uint8 [256,3], lo, hi:  t = (bA * sA + bB * sB) + bC * sC;  HSR_EXPORT_DEPTH's index rule:
 *   u = (t - lo) / (hi - lo);  u = u > 0 ? (u < 1 ? u : 1) : 0 (a NaN gives 0);  idx = (int)(u * 255.0f);  table[idx], lit as above.
 *
 * Every index is checked before it is used: f against F, the face's vertices against V, a label against n; idx is 0..255 by
 * construction and n == 256 is required.  A face image from another mesh, or a mesh with wild indices, gives background or black
 * pixels and never a read out of bounds.
 *
 * Refused: what hsr_mesh_depth refuses of V, F, H, W, fx, fy, cx, cy; a NULL w2c or face_image; a NULL vertices or faces with F > 0;
 * n_jobs outside 1..HSR_SHADE_MAX_JOBS or a NULL jobs; per job: an unknown kind; a NULL out; a NULL attr for COLOUR, LABELS, SCALAR; a
 * NULL table for LABELS, SCALAR; n < 1 for LABELS; n != 256 for SCALAR; hi - lo not finite or not positive for SCALAR; ambient not
 * finite or outside [0, 1].  Fields a kind does not name are not read.  No output may overlap an input or another output.
 *
 * The kernel takes 4 consecutive pixels of the flat index a lane and writes 12 bytes per picture and lane; when an out is not 4-byte
 * aligned the whole call takes a one-pixel-per-lane variant with the same results.
 */
#ifndef HSR_MESH_SHADE_H_INCLUDED
#define HSR_MESH_SHADE_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSR_SHADE_MAX_JOBS 8
#define HSR_SHADE_SHADED  0   /* albedo                                               -> out */
#define HSR_SHADE_COLOUR  1   /* attr uint8 [V,3]                                     -> out */
#define HSR_SHADE_NORMALS 2   /*                                                      -> out */
#define HSR_SHADE_LABELS  3   /* attr int32 [V], table uint8 [n,3]                    -> out */
#define HSR_SHADE_SCALAR  4   /* attr float [V], table uint8 [256,3], lo, hi          -> out */

typedef struct hsr_shade_job {
    int kind;
    int lit;                      /* COLOUR, LABELS, SCALAR: multiply by shade */
    const float* normals;         /* [V,3] world space, or NULL: flat shading */
    const void* attr;
    const uint8_t* table;
    int n;                        /* rows of table */
    float lo, hi;
    float ambient;
    float albedo[3];
    uint8_t background[4];        /* R G B; the fourth byte is not read */
    uint8_t* out;                 /* [H,W,3], R G B */
} hsr_shade_job;

size_t hsr_mesh_normals_scratch_bytes(int V);

int hsr_mesh_normals(int V, int F, const float* vertices, const int* faces, void* scratch, size_t scratch_bytes, float* out_normals,
                     void* stream);

/* w2c: HOST array of 16 floats; jobs: HOST array of n_jobs entries */
int hsr_mesh_shade(int V, int F, const float* vertices, const int* faces, int H, int W, float fx, float fy, float cx, float cy,
                   const float* w2c, const int* face_image, int n_jobs, const hsr_shade_job* jobs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSR_MESH_SHADE_H_INCLUDED */
