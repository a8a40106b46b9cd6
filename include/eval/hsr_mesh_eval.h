/*
 * hsr_mesh_eval.h — C ABI of the scoring of a run's mesh against a ground-truth mesh (libhsr_rast.so), DESIGN.md §7 row 15: triangle
 * areas, area-weighted surface samples, the ground-truth vertices the cameras saw, and an EXACT nearest-neighbour search between two
 * point sets on a uniform grid.  The reference has no mesh evaluation (its family leaves the device for Open3D, trimesh or a KD-tree), so
 * nothing here is pinned by reference outputs: every rule below is RESTATED here, and tests/mesh_eval_ref.py restates it once more in
 * numpy for the tests.  The header lives under include/eval/: the prototypes under include/hsr_*.h and include/ext/ are counted sets
 * (tests/test_abi.py); these are bound under this header's key in diff_gaussian_rasterization/_abi.py EVAL_HEADERS.
 *
 * All pointers are DEVICE pointers and contiguous, except `w2c`: a HOST array of 16 floats (row-major world-to-camera, rows 0..2 are
 * read) that is copied into the kernel arguments by value.  Everything runs on `stream`; no entry point allocates or synchronises with
 * the host.  Every refusal returns HSR_ERR_INVALID_ARGUMENT (-1) before any device work, with a message in hsr_last_error()
 * (hsr_rasterizer.h) that starts "mesh_areas: ", "mesh_sample: ", "mesh_seen: ", "nn_cells: ", "nn_pack: " or "nn_query: ".  A count of
 * 0 items launches nothing.  No kernel here waits for another workgroup and none uses an atomic: every output element has one owner.
 * The file is built without contraction: every float32 operation below is rounded once, in exactly the stated order, and the numpy
 * restatement matches bit for bit.
 *
 * hsr_mesh_areas — F faces int32 [F,3] over V vertices float32 [V,3], with A, B, C the corners of a face:
 *   e1 = B - A,  e2 = C - A,  c = (e1y * e2z - e1z * e2y,  e1z * e2x - e1x * e2z,  e1x * e2y - e1y * e2x)
 *   out_area[f] = 0.5f * sqrtf((cx * cx + cy * cy) + cz * cz)
 * A face with a vertex index outside 0..V-1, or whose area is not finite, gets 0 and is therefore never sampled.
 * Refused: V < 1, F < 0, a NULL pointer with F > 0.
 *
 * hsr_mesh_sample — S points on the surface, the faces chosen in proportion to their areas.  `cum` float64 [F] is the INCLUSIVE running
 * sum of the areas (torch.cumsum(area.double(), 0)); total = cum[F-1].  Sample s draws three 64-bit words z_k, k = 0, 1, 2, from the
 * splitmix64 finaliser (all arithmetic modulo 2^64):
 *   z = seed + (3 * s + k + 1) * 0x9E3779B97F4A7C15;  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *   z ^= z >> 31
 *   face    x = ((double)(z_0 >> 11) * 2^-53) * total;  f = the first face with cum[f] > x, by binary search; when there is none (x
 *           rounded up to total), the first face with cum[f] == total.  A face of area 0 has cum[f] == cum[f-1] and is never the first.
 *   point   u1 = (float)(z_1 >> 40) * 2^-24,  u2 likewise from z_2;  r = sqrtf(u1),  a = 1 - r,  b = r * (1 - u2),  c = r * u2
 *           out_points[s] = (a * A + b * B) + c * C per coordinate                                   float32 [S,3]
 *   out_face[s] = f                                                                                   int32 [S]
 *   out_label[s] = vertex_labels[corner with the largest of (a, b, c), the first on a tie]            int32 [S]
 * vertex_labels int32 [V] and out_label are optional, NULL together.  A chosen face with an index outside 0..V-1 (a `cum` that is not
 * this mesh's) reads nothing: its point is NaN and its label -1.  `seed` is a 64-bit word (size_t).
 * Refused: V < 1, F < 1, S < 0, a NULL vertices, faces, cum, out_points or out_face with S > 0, vertex_labels without out_label or the
 * reverse.  The caller checks total > 0 on the host, from the one read of cum[F-1] it needs anyway.
 *
 * hsr_mesh_seen — one view per launch, as hsr_tsdf_integrate.  seen uint8 [V] is set to 1, and never cleared, where the vertex p
 * projects into the H x W image by the chain of ext/hsr_tsdf.h (hsr_tsdf_integrate, with p for the sample point; both kernels call
 * the one device function of csrc/hsr_project.h):
 *   xc = ((m00 * px + m01 * py) + m02 * pz) + m03, likewise yc and zc;                               not seen unless zc > 0
 *   u = fx * (xc / zc) + cx,  v = fy * (yc / zc) + cy;  fu = floorf(u + 0.5f),  fv = floorf(v + 0.5f)
 *   not seen unless 0 <= fu < W and 0 <= fv < H, tested in float BEFORE the conversion;  pix = (int)fv * W + (int)fu
 *   depth given (float32 [H,W]):  d = depth[pix];  not seen unless d > 0, d is finite and zc <= d + eps
 * Refused: V < 0, H or W outside 1..HSR_MESH_MAX_IMAGE_SIDE, eps not finite or negative, a NULL w2c, or a NULL vertices or seen with V > 0.
 *
 * The grid of the search: origin o, cell size c, sides X, Y, Z; cell (i, j, k) has the number (k * Y + j) * X + i.  A point p goes to
 * the cell, per axis,
 *   f = floorf((p - o) / c);  i = f >= X ? X - 1 : (f > 0 ? (int)f : 0)          a NaN goes to 0, a point outside the box to its edge
 * Refused by the three entry points that take a grid: a side outside 1..HSR_NN_MAX_SIDE, X * Y * Z > HSR_NN_MAX_CELLS (2^24), c not
 * finite and positive, o not finite.
 *
 * hsr_nn_cells — out_cell int32 [M]: the cell number of each of M points float32 [M,3].
 * hsr_nn_pack  — out_packed [M] of 16 bytes each: entry m holds x, y, z of point order[m] and order[m] itself as the bits of the
 *                fourth word; `order` int64 [M] are the indices of torch.sort(cell, stable=True).  A candidate is then ONE 16-byte load.
 *                An order[m] outside 0..M-1 writes a NaN point that never wins.  out_packed must be 16-byte aligned.
 * hsr_nn_query — N queries float32 [N,3] against the M packed points; cell_start int32 [X*Y*Z + 1] is where each cell's points start in
 *                the packed order (torch.searchsorted of 0..X*Y*Z on the sorted cells; cell_start[X*Y*Z] = M).
 *   The RESULT is defined by brute force, not by the search.  For a query q and a point p, in float32:
 *     d = q - p per coordinate,  d2 = (dx * dx + dy * dy) + dz * dz
 *     out_d2[n]    = the least d2 over all M points                                                   float32 [N]
 *     out_index[n] = the smallest original index among the points that reach it                       int32 [N]
 *   Only a d2 < +inf can win: a query or a point with a NaN never does, and a query with no winner gets +inf and -1.
 *   The SEARCH, one lane per query: the cells at Chebyshev distance r = 0, 1, 2, ... from the query's own (clamped) cell, clipped to
 *   the grid.  It stops after ring r >= 1 when  best_d2 <= t * t  with  t = ((float)r - 1/64) * c  (float32), and after the ring that
 *   has covered the grid.  A query with a coordinate that is not finite has no winner and searches nothing.
 *   Why the slack of 1/64 cell makes the search exact.  After ring r every point whose cell is within r of the query's cell on all
 *   three axes has been compared.  Take a point that has not: on some axis its cell index differs from the query's, qi, by at least
 *   r + 1; say it is >= qi + r + 1 (the other side mirrors).  Then qi + r + 1 <= X - 1, so qi < X - 1: the query was not clamped from
 *   above on this axis, and whether it was clamped from below (it lies under o; its projection onto the box lies in cell 0 = qi) or
 *   not, its coordinate is below the upper face of cell qi, o + (qi + 1) * c.  The point — clamped or not — lies at or above the lower
 *   face of its cell, o + (qi + r + 1) * c.  In exact arithmetic the two are therefore more than r * c apart on this axis alone.  The
 *   cell assignment rounds twice, the subtraction and the division, each by at most 2^-24 of a quotient below 1024 = 2^10 cells, so a
 *   coordinate may sit up to 2^-13 cell on the wrong side of a face, about 2^-12 cell for the pair; d2 itself is rounded three times
 *   (relative 2^-22 at most), and t * t twice.  All of that is below 2^-11 cell, 32 times less than the slack: an uncompared point has
 *   d2 > t * t >= best_d2 strictly, so it can neither beat the winner nor tie with it under a smaller index.  At r = 0 the bound would
 *   be negative and its square meaningless: hence r >= 1.
 *   cell_start entries are clamped into 0..M before they are followed, so a table that is not this packing's reads nothing out of bounds.
 *   Refused: N < 0, M < 1, a NULL pointer with N > 0, packed not 16-byte aligned.
 */
#ifndef HSR_MESH_EVAL_H_INCLUDED
#define HSR_MESH_EVAL_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#define HSR_MESH_MAX_IMAGE_SIDE 16384
#define HSR_NN_MAX_SIDE 1024
#define HSR_NN_MAX_CELLS 16777216

#ifdef __cplusplus
extern "C" {
#endif

int hsr_mesh_areas(int V, int F, const float* vertices, const int* faces, float* out_area, void* stream);

int hsr_mesh_sample(int V, int F, int S, size_t seed, const float* vertices, const int* faces, const double* cum,
                    const int* vertex_labels, float* out_points, int* out_face, int* out_label, void* stream);

int hsr_mesh_seen(int V, const float* vertices, int H, int W, float fx, float fy, float cx, float cy, const float* w2c,
                  const float* depth, float eps, uint8_t* seen, void* stream);

int hsr_nn_cells(int X, int Y, int Z, float ox, float oy, float oz, float c, int M, const float* points, int* out_cell, void* stream);

int hsr_nn_pack(int M, const float* points, const int64_t* order, void* out_packed, void* stream);

int hsr_nn_query(int X, int Y, int Z, float ox, float oy, float oz, float c, int M, const int* cell_start, const void* packed,
                 int N, const float* queries, float* out_d2, int* out_index, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSR_MESH_EVAL_H_INCLUDED */
