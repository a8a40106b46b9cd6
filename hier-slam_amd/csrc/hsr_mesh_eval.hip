// hsr_mesh_eval.hip — the scoring of a run's mesh against a ground-truth mesh (gfx950): triangle areas, area-weighted surface samples,
// the vertices a view saw, and an exact nearest-neighbour search on a uniform grid (include/eval/hsr_mesh_eval.h, which states every
// rule; the reference has no mesh evaluation, so the rules are restated there and not pinned by reference outputs).
//   areas  : areas_kernel — a face per lane: three gathered vertices, one cross product.
//   sample : sample_kernel — a sample per lane: three splitmix64 words, a binary search of the float64 running sum (log2 F dependent
//            loads of a table every lane shares, so it stays in cache), three gathered vertices.
//   seen   : seen_kernel — a vertex per lane and one view per launch: hsr_tsdf_integrate's projection (hsr_project.h, the one function
//            both files call), one gathered depth, a byte written only where it becomes 1.
//   cells  : cells_kernel — a point per lane.      pack : pack_kernel — a packed entry per lane, one gathered point, one 16-byte store.
//   query  : query_kernel — a query per lane.  The caller hands the queries over sorted by their own cell, so the 64 lanes of a wave
//            stand in the same or neighbouring cells: they walk the same rows of the grid, the cell_start words and the packed
//            candidates they load are the same lines, and their ring counts — the one divergent loop bound — agree.  A row of the grid
//            (fixed j, k) is contiguous in the packed order, so a ring costs two cell_start loads per row and then one 16-byte load per
//            candidate.  No LDS, no cross-lane traffic; the kernel is a latency-bound gather that lives on occupancy.  The grid, a
//            point's cell, the scan of a row and the ring walk itself are in hsr_nn_grid.h, which hsr_mesh_align.hip includes too.
// Compiled with -ffp-contract=off: every output is pinned bit for bit against a numpy restatement that rounds every operation once.
#include <math.h>

#include "hsr_common.h"
#include "hsr_nn_grid.h"
#include "hsr_project.h"
#include "../../include/eval/hsr_mesh_eval.h"

namespace {

constexpr int TB = 256;

struct View {
    float m[12];      // rows 0..2 of the world-to-camera matrix
    float fx, fy, cx, cy;
    int H, W;
    float eps;
};

// ---- areas and samples ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void areas_kernel(int V, int F, const float* __restrict__ vertices, const int* __restrict__ faces,
                                                   float* __restrict__ out_area)
{
    const int f = blockIdx.x * TB + threadIdx.x;
    if (f >= F) return;
    const int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
    float area = 0.f;
    if ((unsigned)ia < (unsigned)V && (unsigned)ib < (unsigned)V && (unsigned)ic < (unsigned)V) {
        const float* A = vertices + 3 * (size_t)ia;
        const float* B = vertices + 3 * (size_t)ib;
        const float* C = vertices + 3 * (size_t)ic;
        const float e1x = B[0] - A[0], e1y = B[1] - A[1], e1z = B[2] - A[2];
        const float e2x = C[0] - A[0], e2y = C[1] - A[1], e2z = C[2] - A[2];
        const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
        area = 0.5f * sqrtf((cx * cx + cy * cy) + cz * cz);
        if (!(area < INFINITY)) area = 0.f;      // a NaN fails the comparison too
    }
    out_area[f] = area;
}

__device__ __forceinline__ unsigned long long splitmix(unsigned long long seed, unsigned long long n)
{
    unsigned long long z = seed + n * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(TB) void sample_kernel(int V, int F, int S, unsigned long long seed, const float* __restrict__ vertices,
                                                    const int* __restrict__ faces, const double* __restrict__ cum,
                                                    const int* __restrict__ vertex_labels, float* __restrict__ out_points,
                                                    int* __restrict__ out_face, int* __restrict__ out_label)
{
    const int s = blockIdx.x * TB + threadIdx.x;
    if (s >= S) return;
    const unsigned long long n = 3ull * (unsigned long long)s;
    const unsigned long long z0 = splitmix(seed, n + 1), z1 = splitmix(seed, n + 2), z2 = splitmix(seed, n + 3);
    const double total = cum[F - 1];
    const double x = ((double)(z0 >> 11) * 0x1p-53) * total;
    // the first f with cum[f] > x; F when there is none
    int lo = 0, hi = F;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (cum[mid] > x) hi = mid; else lo = mid + 1;
    }
    if (lo == F) {      // x was rounded up to the total: the first f with cum[f] >= total, which is the last face with an area
        lo = 0; hi = F - 1;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (cum[mid] >= total) hi = mid; else lo = mid + 1;
        }
    }
    const int f = lo;
    const float u1 = (float)(z1 >> 40) * 0x1p-24f, u2 = (float)(z2 >> 40) * 0x1p-24f;
    const float r = sqrtf(u1);
    const float a = 1.f - r, b = r * (1.f - u2), c = r * u2;
    const int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
    const bool ok = (unsigned)ia < (unsigned)V && (unsigned)ib < (unsigned)V && (unsigned)ic < (unsigned)V;
    float p[3] = {NAN, NAN, NAN};
    int label = -1;
    if (ok) {
        const float* A = vertices + 3 * (size_t)ia;
        const float* B = vertices + 3 * (size_t)ib;
        const float* C = vertices + 3 * (size_t)ic;
#pragma unroll
        for (int q = 0; q < 3; q++) p[q] = (a * A[q] + b * B[q]) + c * C[q];
        if (vertex_labels) label = vertex_labels[a >= b ? (a >= c ? ia : ic) : (b >= c ? ib : ic)];
    }
#pragma unroll
    for (int q = 0; q < 3; q++) out_points[3 * (size_t)s + q] = p[q];
    out_face[s] = f;
    if (out_label) out_label[s] = label;
}

// ---- seen -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void seen_kernel(View c, int V, const float* __restrict__ vertices, const float* __restrict__ depth,
                                                  uint8_t* __restrict__ seen)
{
    const int v = blockIdx.x * TB + threadIdx.x;
    if (v >= V) return;
    const float px = vertices[3 * (size_t)v], py = vertices[3 * (size_t)v + 1], pz = vertices[3 * (size_t)v + 2];
    float zc;
    int pix;
    if (!hsr_project_pixel(c.m, c.fx, c.fy, c.cx, c.cy, c.H, c.W, px, py, pz, zc, pix)) return;      // hsr_tsdf_integrate's chain: hsr_project.h
    if (depth) {
        const float d = depth[pix];
        if (!(d > 0.f && d < INFINITY && zc <= d + c.eps)) return;
    }
    seen[v] = 1;
}

// ---- the grid ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void cells_kernel(Grid g, int M, const float* __restrict__ points, int* __restrict__ out_cell)
{
    const int m = blockIdx.x * TB + threadIdx.x;
    if (m >= M) return;
    const int i = cell_axis(points[3 * (size_t)m], g.ox, g.c, g.X), j = cell_axis(points[3 * (size_t)m + 1], g.oy, g.c, g.Y);
    const int k = cell_axis(points[3 * (size_t)m + 2], g.oz, g.c, g.Z);
    out_cell[m] = (k * g.Y + j) * g.X + i;
}

__global__ __launch_bounds__(TB) void pack_kernel(int M, const float* __restrict__ points, const long long* __restrict__ order,
                                                  f4* __restrict__ out_packed)
{
    const int m = blockIdx.x * TB + threadIdx.x;
    if (m >= M) return;
    const long long src = order[m];
    f4 e = {NAN, NAN, NAN, __int_as_float(-1)};
    if (src >= 0 && src < (long long)M) {
        e[0] = points[3 * src];
        e[1] = points[3 * src + 1];
        e[2] = points[3 * src + 2];
        e[3] = __int_as_float((int)src);
    }
    out_packed[m] = e;
}

__global__ __launch_bounds__(TB) void query_kernel(Grid g, int M, const int* __restrict__ cell_start, const f4* __restrict__ packed, int N,
                                                   const float* __restrict__ queries, float* __restrict__ out_d2, int* __restrict__ out_index)
{
    const int n = blockIdx.x * TB + threadIdx.x;
    if (n >= N) return;
    const float qx = queries[3 * (size_t)n], qy = queries[3 * (size_t)n + 1], qz = queries[3 * (size_t)n + 2];
    Best best{INFINITY, 0x7fffffff, 0};
    if (fabsf(qx) < INFINITY && fabsf(qy) < INFINITY && fabsf(qz) < INFINITY)      // else every d2 is +inf or a NaN: nothing to search
        best = ring_walk<false>(g, M, cell_start, packed, qx, qy, qz, 0.f);      // hsr_nn_grid.h
    const bool won = best.d2 < INFINITY;
    out_d2[n] = won ? best.d2 : INFINITY;
    out_index[n] = won ? best.index : -1;
}

unsigned blocks_for(int items) { return (unsigned)(((long long)items + TB - 1) / TB); }

}  // namespace

extern "C" int hsr_mesh_areas(int V, int F, const float* vertices, const int* faces, float* out_area, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (V < 1 || F < 0) {
        hsr_set_error("mesh_areas: invalid sizes V=%d F=%d (V >= 1, F >= 0)", V, F);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (F > 0 && (!vertices || !faces || !out_area)) {
        hsr_set_error("mesh_areas: vertices, faces and out_area are required with F > 0");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (F == 0) return HSR_OK;
    areas_kernel<<<blocks_for(F), TB, 0, stream>>>(V, F, vertices, faces, out_area);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_mesh_sample(int V, int F, int S, size_t seed, const float* vertices, const int* faces, const double* cum,
                               const int* vertex_labels, float* out_points, int* out_face, int* out_label, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (V < 1 || F < 1 || S < 0) {
        hsr_set_error("mesh_sample: invalid sizes V=%d F=%d S=%d (V >= 1, F >= 1, S >= 0)", V, F, S);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if ((vertex_labels == nullptr) != (out_label == nullptr)) {
        hsr_set_error("mesh_sample: vertex_labels and out_label come together");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (S > 0 && (!vertices || !faces || !cum || !out_points || !out_face)) {
        hsr_set_error("mesh_sample: vertices, faces, cum, out_points and out_face are required with S > 0");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (S == 0) return HSR_OK;
    sample_kernel<<<blocks_for(S), TB, 0, stream>>>(V, F, S, (unsigned long long)seed, vertices, faces, cum, vertex_labels, out_points, out_face,
                                                    out_label);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_mesh_seen(int V, const float* vertices, int H, int W, float fx, float fy, float cx, float cy, const float* w2c,
                             const float* depth, float eps, uint8_t* seen, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (V < 0) {
        hsr_set_error("mesh_seen: invalid size V=%d (V >= 0)", V);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (H < 1 || W < 1 || H > HSR_MESH_MAX_IMAGE_SIDE || W > HSR_MESH_MAX_IMAGE_SIDE) {
        hsr_set_error("mesh_seen: invalid image size H=%d W=%d (1..%d)", H, W, HSR_MESH_MAX_IMAGE_SIDE);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!(isfinite(eps) && eps >= 0.f)) {
        hsr_set_error("mesh_seen: eps must be finite and not negative; got %g", (double)eps);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!w2c || (V > 0 && (!vertices || !seen))) {
        hsr_set_error("mesh_seen: w2c (16 floats on the host) is required, and vertices and seen with V > 0");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (V == 0) return HSR_OK;
    View c;
    for (int q = 0; q < 12; q++) c.m[q] = w2c[q];
    c.fx = fx; c.fy = fy; c.cx = cx; c.cy = cy;
    c.H = H; c.W = W;
    c.eps = eps;
    seen_kernel<<<blocks_for(V), TB, 0, stream>>>(c, V, vertices, depth, seen);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_nn_cells(int X, int Y, int Z, float ox, float oy, float oz, float c, int M, const float* points, int* out_cell,
                            void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (bad_grid("nn_cells", X, Y, Z, ox, oy, oz, c)) return HSR_ERR_INVALID_ARGUMENT;
    if (M < 0 || (M > 0 && (!points || !out_cell))) {
        hsr_set_error("nn_cells: M=%d must be >= 0, and points and out_cell are required with M > 0", M);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (M == 0) return HSR_OK;
    cells_kernel<<<blocks_for(M), TB, 0, stream>>>(Grid{X, Y, Z, ox, oy, oz, c}, M, points, out_cell);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_nn_pack(int M, const float* points, const int64_t* order, void* out_packed, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (M < 0 || (M > 0 && (!points || !order || !out_packed))) {
        hsr_set_error("nn_pack: M=%d must be >= 0, and points, order and out_packed are required with M > 0", M);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!aligned16(out_packed)) {
        hsr_set_error("nn_pack: out_packed must be 16-byte aligned");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (M == 0) return HSR_OK;
    pack_kernel<<<blocks_for(M), TB, 0, stream>>>(M, points, reinterpret_cast<const long long*>(order), reinterpret_cast<f4*>(out_packed));
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_nn_query(int X, int Y, int Z, float ox, float oy, float oz, float c, int M, const int* cell_start, const void* packed,
                            int N, const float* queries, float* out_d2, int* out_index, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (bad_grid("nn_query", X, Y, Z, ox, oy, oz, c)) return HSR_ERR_INVALID_ARGUMENT;
    if (N < 0 || M < 1) {
        hsr_set_error("nn_query: invalid sizes N=%d M=%d (N >= 0, M >= 1)", N, M);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (N > 0 && (!cell_start || !packed || !queries || !out_d2 || !out_index)) {
        hsr_set_error("nn_query: cell_start, packed, queries, out_d2 and out_index are required with N > 0");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!aligned16(packed)) {
        hsr_set_error("nn_query: packed must be 16-byte aligned");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (N == 0) return HSR_OK;
    query_kernel<<<blocks_for(N), TB, 0, stream>>>(Grid{X, Y, Z, ox, oy, oz, c}, M, cell_start, reinterpret_cast<const f4*>(packed), N, queries,
                                                   out_d2, out_index);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}
