// hsr_nn_grid.h — the uniform grid of the nearest-neighbour searches (internal, not part of the C ABI): the grid's numbers, a point's
// cell, the scan of a row's packed candidates, the ring walk and the grid's refusals, once, for hsr_mesh_eval.hip (hsr_nn_cells,
// hsr_nn_query) and hsr_mesh_align.hip (hsr_icp_step), so that the two searches cannot drift apart.  include/eval/hsr_mesh_eval.h states
// the rules and proves the stopping rule; include/align/hsr_mesh_align.h states the one more rule of the capped walk.  Every device
// function is __device__ __forceinline__, so the including file's flags (-ffp-contract=off for both includers) apply to the inlined
// code.  Everything is in an anonymous namespace: each includer gets its own internal copy, as when the code stood in its file.
#pragma once
#include <math.h>

#include "hsr_common.h"
#include "../../include/eval/hsr_mesh_eval.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

struct Grid {
    int X, Y, Z;
    float ox, oy, oz, c;
};

__device__ __forceinline__ int cell_axis(float p, float o, float c, int n)
{
    const float f = floorf((p - o) / c);
    return f >= (float)n ? n - 1 : (f > 0.f ? (int)f : 0);      // a NaN fails both comparisons: 0
}

struct Best {
    float d2;
    int index;
    int at;      // where the winner stands in the packed order (hsr_icp_step gathers it; hsr_nn_query never reads it)
};

// the packed points of cells a..b of one row (consecutive numbers) against the query
__device__ __forceinline__ void scan_cells(int a, int b, int M, const int* __restrict__ cell_start, const f4* __restrict__ packed, float qx,
                                           float qy, float qz, Best& best)
{
    int begin = cell_start[a], end = cell_start[b + 1];
    begin = begin < 0 ? 0 : begin;
    end = end > M ? M : end;
    for (int m = begin; m < end; m++) {
        const f4 p = packed[m];
        const float dx = qx - p[0], dy = qy - p[1], dz = qz - p[2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const int index = __float_as_int(p[3]);
        if (d2 < best.d2 || (d2 == best.d2 && index < best.index)) {      // a NaN fails both
            best.d2 = d2;
            best.index = index;
            best.at = m;
        }
    }
}

// The ring walk around the clamped cell of the query (qx, qy, qz), whose coordinates are finite: the rings r = 0, 1, 2, ... clipped to
// the grid, until  best.d2 <= t * t  with  t = ((float)r - 1/64) * c  after a ring r >= 1, or the ring has covered the grid.  CAPPED adds
// the stop  m2 <= t * t  (hsr_mesh_align.h): nothing farther than sqrt(m2) is of interest, and the caller discards a best beyond it.
template <bool CAPPED>
__device__ __forceinline__ Best ring_walk(const Grid& g, int M, const int* __restrict__ cell_start, const f4* __restrict__ packed, float qx,
                                          float qy, float qz, float m2)
{
    Best best{INFINITY, 0x7fffffff, 0};
    const int qi = cell_axis(qx, g.ox, g.c, g.X), qj = cell_axis(qy, g.oy, g.c, g.Y), qk = cell_axis(qz, g.oz, g.c, g.Z);
    for (int r = 0;; r++) {
        const int i0 = max(qi - r, 0), i1 = min(qi + r, g.X - 1);
        const int j0 = max(qj - r, 0), j1 = min(qj + r, g.Y - 1);
        const int k0 = max(qk - r, 0), k1 = min(qk + r, g.Z - 1);
        for (int k = k0; k <= k1; k++) {
            const bool k_face = k == qk - r || k == qk + r;
            for (int j = j0; j <= j1; j++) {
                const int row = (k * g.Y + j) * g.X;
                if (k_face || j == qj - r || j == qj + r) {
                    scan_cells(row + i0, row + i1, M, cell_start, packed, qx, qy, qz, best);      // a row of the ring's shell
                } else {                                                                            // inside it: the two end cells
                    if (qi - r >= 0) scan_cells(row + qi - r, row + qi - r, M, cell_start, packed, qx, qy, qz, best);
                    if (qi + r < g.X) scan_cells(row + qi + r, row + qi + r, M, cell_start, packed, qx, qy, qz, best);
                }
            }
        }
        if (r >= 1) {
            const float t = ((float)r - 0.015625f) * g.c;
            if (best.d2 <= t * t) break;
            if (CAPPED && m2 <= t * t) break;
        }
        if (i0 == 0 && j0 == 0 && k0 == 0 && i1 == g.X - 1 && j1 == g.Y - 1 && k1 == g.Z - 1) break;      // the ring covered the grid
    }
    return best;
}

inline bool finite_positive(float x) { return isfinite(x) && x > 0.f; }

inline bool bad_grid(const char* who, int X, int Y, int Z, float ox, float oy, float oz, float c)
{
    const bool sides = X >= 1 && Y >= 1 && Z >= 1 && X <= HSR_NN_MAX_SIDE && Y <= HSR_NN_MAX_SIDE && Z <= HSR_NN_MAX_SIDE;
    if (!sides || (long long)X * Y * Z > (long long)HSR_NN_MAX_CELLS) {
        hsr_set_error("%s: invalid grid X=%d Y=%d Z=%d (every side 1..%d, X*Y*Z <= 2^24)", who, X, Y, Z, HSR_NN_MAX_SIDE);
        return true;
    }
    if (!finite_positive(c) || !isfinite(ox) || !isfinite(oy) || !isfinite(oz)) {
        hsr_set_error("%s: the cell size must be finite and positive and the origin finite; got %g and (%g, %g, %g)", who, (double)c, (double)ox,
                      (double)oy, (double)oz);
        return true;
    }
    return false;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
