/*
 * hsr_mesh_align.h — C ABI of the registration of a run's mesh to the ground truth before it is scored (libhsr_rast.so), DESIGN.md §7
 * row 19: ONE pass of rigid point-to-point ICP — transform the source points, find each one's exact nearest target within the
 * correspondence distance, and reduce the seventeen sums the closed-form (Horn / Kabsch) solve needs — in one launch plus a
 * one-workgroup reduction.  The published tables of this family register with Open3D's registration_icp; Open3D is not a dependency and
 * the reference has no mesh evaluation, so nothing here is pinned by outside outputs: every rule below is RESTATED here, and
 * tests/mesh_align_ref.py restates it once more in numpy for the tests.  The header lives under include/align/: the prototypes under
 * include/hsr_*.h, include/ext/, include/eval/, include/recon/, include/sensor/ and include/surface/ are counted sets; these are bound
 * under this header's key in diff_gaussian_rasterization/_abi.py ALIGN_HEADERS.
 *
 * All pointers are DEVICE pointers and contiguous, except `transform`: a HOST array of 12 floats (rows 0..2 of a row-major 4 x 4) that
 * is copied into the kernel arguments by value.  Everything runs on `stream`; no entry point allocates or synchronises with the host.
 * Every refusal returns HSR_ERR_INVALID_ARGUMENT (-1) before any device work, with a message in hsr_last_error() (hsr_rasterizer.h)
 * that starts "icp_step: ".  No kernel here waits for another workgroup and none uses an atomic: every output element has one owner.
 * The file is built without contraction: every float32 operation below is rounded once, in exactly the stated order.
 *
 * hsr_icp_scratch_bytes — the bytes of `scratch` hsr_icp_step needs for N source points: one row of 17 float64 per 256 points.
 *   0 for N <= 0.
 *
 * hsr_icp_step — the grid (X, Y, Z, ox, oy, oz, c), M, cell_start and packed are exactly those of hsr_nn_query
 * (eval/hsr_mesh_eval.h): the TARGET points.  source float32 [N,3];  max_dist the correspondence distance.
 *   The RESULT is defined by brute force, not by the search.  For a source point p and the transform m, in float32:
 *     x' = ((m00 * px + m01 * py) + m02 * pz) + m03,  likewise y' (m10..m13) and z' (m20..m23)
 *     (d2, index) = hsr_nn_query's answer for the query p' = (x', y', z'): the least (dx * dx + dy * dy) + dz * dz over ALL M points,
 *                   the smallest original index on a tie; a NaN never wins, and only a d2 < +inf can
 *     m2 = max_dist * max_dist
 *   p has a CORRESPONDENCE iff there is a winner and d2 <= m2.  Then
 *     out_d2[n] = d2,  out_index[n] = index                          float32 [N], int32 [N]; otherwise +inf and -1
 *   out_index and out_d2 are optional and are NULL together.
 *   out_sums float64 [17], over the points with a correspondence, q being the winning target point, everything converted to float64
 *   BEFORE it is multiplied or added:
 *     [0] their number   [1..3] sum of p'   [4..6] sum of q   [7 + 3 * a + b] sum of p'_a * q_b   [16] sum of d2
 *   The number is exact.  The other additions are made in an order of the implementation's own that depends on N alone: the butterfly
 *   of a wave, the four waves of a workgroup in ascending order, and the workgroups' rows by a fixed split (row b goes to part b mod 15,
 *   a part adds its rows in ascending order, the parts are added in ascending order).  Equal inputs give equal bytes on every run.
 *   N = 0 launches nothing except what writes 17 zeros.
 *   The SEARCH is hsr_nn_query's ring walk (one function, csrc/hsr_nn_grid.h) with one more stopping rule: after ring r >= 1, with
 *   t = ((float)r - 1/64) * c, it stops when  best_d2 <= t * t  OR  m2 <= t * t.  Why the second stop is exact: hsr_mesh_eval.h
 *   proves that after ring r every point not yet compared has d2 > t * t strictly; once t * t >= m2 no such point can be a
 *   correspondence, a best with d2 <= m2 <= t * t is the exact answer by the first rule's own proof, and a best with d2 > m2 is
 *   reported as none — which is what brute force reports, since its least d2 is then either this best or a d2 > t * t >= m2.
 *   A source point far from every target therefore costs ceil(max_dist / c) + 1 rings, not the whole grid.
 *   A source point whose transformed coordinates are not all finite has no correspondence and searches nothing.
 *   The caller hands the source points over sorted by the cell of their transformed position — once per ICP run, not once per pass: the
 *   motion between passes is a fraction of a cell — so that a wave's lanes walk the same rows.  Speed only: any order gives the same
 *   out_d2 and out_index per point and the same number.
 *   Refused: what hsr_nn_query refuses (a side outside 1..HSR_NN_MAX_SIDE, X * Y * Z > HSR_NN_MAX_CELLS, c not finite and positive, o
 *   not finite, N < 0, M < 1, a NULL cell_start, packed or source with N > 0, packed not 16-byte aligned); a NULL transform; a
 *   transform entry that is not finite; a max_dist that is not finite and positive; a NULL out_sums; one of out_index / out_d2 without
 *   the other; with N > 0 a scratch that is NULL, not 8-byte aligned or smaller than hsr_icp_scratch_bytes(N).
 */
#ifndef HSR_MESH_ALIGN_H_INCLUDED
#define HSR_MESH_ALIGN_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#define HSR_ICP_SUMS 17

#ifdef __cplusplus
extern "C" {
#endif

size_t hsr_icp_scratch_bytes(int N);

int hsr_icp_step(int X, int Y, int Z, float ox, float oy, float oz, float c, int M, const int* cell_start, const void* packed,
                 int N, const float* source, const float* transform, float max_dist, int* out_index, float* out_d2,
                 double* out_sums, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSR_MESH_ALIGN_H_INCLUDED */
