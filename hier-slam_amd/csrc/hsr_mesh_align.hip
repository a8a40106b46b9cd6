// hsr_mesh_align.hip — one pass of rigid point-to-point ICP between a run's mesh samples and the ground truth's (gfx950): the transform,
// the exact nearest target within the correspondence distance and the seventeen sums of the closed-form solve, fused
// (include/align/hsr_mesh_align.h, which states every rule; nothing is pinned by outside outputs, so the rules are restated there).
//   step  : icp_step_kernel — a source point per lane, 256-lane workgroups.  The caller hands the source points over sorted by the cell
//           of their transformed position, ONCE per ICP run: the motion between passes is a fraction of a cell, so the 64 lanes of a
//           wave keep standing in the same or neighbouring cells, walk the same rows of the grid, load the same cell_start words and
//           packed candidates, and their ring counts — the one divergent loop bound — agree.  The walk is hsr_nn_query's
//           (hsr_nn_grid.h, one function for both) with the cap: a lane with no target nearby stops after ceil(max_dist / c) + 1 rings
//           instead of walking the grid, so a floater no longer holds its wave.  The winner's point is gathered once more from the
//           packed order (a line the lane has just read), 17 float64 accumulators per lane (zero without a correspondence) go through
//           hsr_block256_sums, and the workgroup writes ONE row of 17 partials.  Latency-bound gather that lives on occupancy, as the
//           query; the float64 tail is 17 butterflies per wave and does not show beside it.
//   sums  : icp_sums_kernel — one workgroup: thread t < 255 adds the rows b = t / 17, t / 17 + 15, ... of column t % 17 in ascending
//           order, then thread k < 17 adds the 15 parts of column k in ascending order.  A fixed order that depends on N alone.
// No atomics, every output has one owner.  Compiled with -ffp-contract=off: d2, index and the transformed point are pinned bit for bit
// against a numpy restatement that rounds every operation once.
#include <math.h>

#include "hsr_block.h"
#include "hsr_common.h"
#include "hsr_nn_grid.h"
#include "../../include/align/hsr_mesh_align.h"

namespace {

constexpr int TB = 256;
constexpr int SUMS = HSR_ICP_SUMS;
constexpr int PARTS = 15;      // PARTS * SUMS = 255 <= TB

struct Rigid {
    float m[12];      // rows 0..2 of the row-major 4 x 4
};

__global__ __launch_bounds__(TB) void icp_step_kernel(Grid g, Rigid T, float m2, int M, const int* __restrict__ cell_start,
                                                      const f4* __restrict__ packed, int N, const float* __restrict__ source,
                                                      int* __restrict__ out_index, float* __restrict__ out_d2, double* __restrict__ partials)
{
    __shared__ double s_red[4][SUMS];
    const int n = blockIdx.x * TB + threadIdx.x;
    double acc[SUMS];
#pragma unroll
    for (int k = 0; k < SUMS; k++) acc[k] = 0.0;
    if (n < N) {
        const float px = source[3 * (size_t)n], py = source[3 * (size_t)n + 1], pz = source[3 * (size_t)n + 2];
        const float x = ((T.m[0] * px + T.m[1] * py) + T.m[2] * pz) + T.m[3];
        const float y = ((T.m[4] * px + T.m[5] * py) + T.m[6] * pz) + T.m[7];
        const float z = ((T.m[8] * px + T.m[9] * py) + T.m[10] * pz) + T.m[11];
        Best best{INFINITY, 0x7fffffff, 0};
        if (fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY)      // else every d2 is +inf or a NaN: nothing to search
            best = ring_walk<true>(g, M, cell_start, packed, x, y, z, m2);
        const bool has = best.d2 < INFINITY && best.d2 <= m2;
        if (has) {
            const f4 q = packed[best.at];      // best.at < M: it was a loop index of scan_cells
            const double p3[3] = {(double)x, (double)y, (double)z}, q3[3] = {(double)q[0], (double)q[1], (double)q[2]};
            acc[0] = 1.0;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                acc[1 + a] = p3[a];
                acc[4 + a] = q3[a];
#pragma unroll
                for (int b = 0; b < 3; b++) acc[7 + 3 * a + b] = p3[a] * q3[b];
            }
            acc[16] = (double)best.d2;
        }
        if (out_d2) {
            out_d2[n] = has ? best.d2 : INFINITY;
            out_index[n] = has ? best.index : -1;
        }
    }
    hsr_block256_sums(acc, s_red, partials + (size_t)SUMS * blockIdx.x);
}

__global__ __launch_bounds__(TB) void icp_sums_kernel(int rows, const double* __restrict__ partials, double* __restrict__ out_sums)
{
    __shared__ double s_part[PARTS][SUMS];
    const int t = threadIdx.x;
    if (t < PARTS * SUMS) {
        const int part = t / SUMS, k = t % SUMS;
        double s = 0.0;
        for (int b = part; b < rows; b += PARTS) s += partials[(size_t)SUMS * b + k];
        s_part[part][k] = s;
    }
    __syncthreads();
    if (t < SUMS) {
        double s = s_part[0][t];
#pragma unroll
        for (int part = 1; part < PARTS; part++) s += s_part[part][t];
        out_sums[t] = s;
    }
}

size_t rows_for(int N) { return N <= 0 ? 0 : ((size_t)N + TB - 1) / TB; }

}  // namespace

extern "C" size_t hsr_icp_scratch_bytes(int N) { return rows_for(N) * SUMS * sizeof(double); }

extern "C" int hsr_icp_step(int X, int Y, int Z, float ox, float oy, float oz, float c, int M, const int* cell_start, const void* packed,
                            int N, const float* source, const float* transform, float max_dist, int* out_index, float* out_d2,
                            double* out_sums, void* scratch, size_t scratch_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (bad_grid("icp_step", X, Y, Z, ox, oy, oz, c)) return HSR_ERR_INVALID_ARGUMENT;
    if (N < 0 || M < 1) {
        hsr_set_error("icp_step: invalid sizes N=%d M=%d (N >= 0, M >= 1)", N, M);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (N > 0 && (!cell_start || !packed || !source)) {
        hsr_set_error("icp_step: cell_start, packed and source are required with N > 0");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!aligned16(packed)) {
        hsr_set_error("icp_step: packed must be 16-byte aligned");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!transform) {
        hsr_set_error("icp_step: transform (12 floats on the host) is required");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    Rigid T;
    for (int q = 0; q < 12; q++) {
        T.m[q] = transform[q];
        if (!isfinite(T.m[q])) {
            hsr_set_error("icp_step: transform entry %d is not finite (%g)", q, (double)T.m[q]);
            return HSR_ERR_INVALID_ARGUMENT;
        }
    }
    if (!finite_positive(max_dist)) {
        hsr_set_error("icp_step: max_dist must be finite and positive; got %g", (double)max_dist);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!out_sums) {
        hsr_set_error("icp_step: out_sums (17 float64) is required");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if ((out_index == nullptr) != (out_d2 == nullptr)) {
        hsr_set_error("icp_step: out_index and out_d2 come together");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const size_t need = hsr_icp_scratch_bytes(N);
    if (N > 0 && (!scratch || scratch_bytes < need || (reinterpret_cast<uintptr_t>(scratch) & 7) != 0)) {
        hsr_set_error("icp_step: the scratch must hold %zu bytes, 8-byte aligned (%zu given, or NULL)", need, scratch_bytes);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const int rows = (int)rows_for(N);
    double* partials = reinterpret_cast<double*>(scratch);
    if (N > 0) {
        icp_step_kernel<<<(unsigned)rows, TB, 0, stream>>>(Grid{X, Y, Z, ox, oy, oz, c}, T, max_dist * max_dist, M, cell_start,
                                                           reinterpret_cast<const f4*>(packed), N, source, out_index, out_d2, partials);
        HSR_HIP_CHECK(hipGetLastError());
    }
    icp_sums_kernel<<<1, TB, 0, stream>>>(rows, partials, out_sums);      // rows = 0: 17 zeros
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}
