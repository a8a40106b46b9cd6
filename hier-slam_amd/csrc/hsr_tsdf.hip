// hsr_tsdf.hip — the mesh of a finished run (gfx950): rendered depth fused into a truncated signed distance volume, and the volume's
// zero surface by marching tetrahedra (include/ext/hsr_tsdf.h, which states every rule; the reference has no mesher, so the rules are
// restated there and not pinned by reference outputs).
//   integrate : integrate_kernel<V> — a stream over the volume with one gathered image read per point.  V = 4: a lane owns four
//               consecutive lin (consecutive x), projects them first and touches the state only where one of the four is updated: 16-byte
//               loads and stores of tsdf / weight (and cweight, the three colour planes, best, label where the band |sdf| <= trunc is
//               hit), so a wave moves whole lines and the points outside the view cost no volume traffic at all.  V = 1 with equal
//               results for X * Y * Z % 4 != 0 (the colour planes then start off a 16-byte boundary) and for unaligned state: one
//               body on hsr_lane_io.h's hsr_load<V> / hsr_store<V>.
//   count     : count_kernel — a cube per lane: eight weights and signs, the triangle count of its six tetrahedra.
//   faces     : faces_kernel — the same walk, writing edge keys at the cube's offset.  Both read each point eight times; the lines are
//               shared by neighbouring lanes and rows, and the pass runs once per mesh, not once per view.
//   vertices  : vertices_kernel — a key per lane: the two endpoints' tsdf (colour, weight, label) and the interpolated vertex.
// Compiled with -ffp-contract=off: integrate and vertices are pinned against a float32 restatement that rounds every operation once.
#include <math.h>

#include "hsr_common.h"
#include "hsr_lane_io.h"
#include "hsr_project.h"
#include "../../include/ext/hsr_tsdf.h"

namespace {

constexpr int TB = 256;

struct Grid {
    int X, Y, Z;
    float ox, oy, oz, h;
};

struct View {
    float m[12];      // rows 0..2 of the world-to-camera matrix
    float fx, fy, cx, cy;
    int H, W;
    float sil_thres, depth_max, trunc, max_weight;
};

struct State {
    float *tsdf, *weight, *color, *cweight, *best;
    int* label;
};

// ---- integrate -------------------------------------------------------------------------------------------------------------------------
// the header's chain for point (i, j, k) up to sdf: false where the point is skipped
__device__ __forceinline__ bool project(const Grid& g, const View& c, int i, int j, int k, const float* __restrict__ depth,
                                        const float* __restrict__ opacity, float& sdf, int& pix)
{
    const float px = g.ox + g.h * (float)i, py = g.oy + g.h * (float)j, pz = g.oz + g.h * (float)k;
    float zc;
    if (!hsr_project_pixel(c.m, c.fx, c.fy, c.cx, c.cy, c.H, c.W, px, py, pz, zc, pix)) return false;      // hsr_project.h
    const float d = depth[pix];
    if (!(d > 0.f && d < INFINITY)) return false;
    if (c.depth_max > 0.f && d > c.depth_max) return false;
    if (opacity && !(opacity[pix] > c.sil_thres)) return false;
    sdf = d - zc;
    return !(sdf < -c.trunc);
}

__device__ __forceinline__ float running_mean(float old, float w, float x) { return (old * w + x) / (w + 1.f); }

template <int V>
__global__ __launch_bounds__(TB) void integrate_kernel(Grid g, View c, long long N, const float* __restrict__ depth,
                                                       const float* __restrict__ image, const long long* __restrict__ labels,
                                                       const float* __restrict__ opacity, State s)
{
    const long long base = ((long long)blockIdx.x * TB + threadIdx.x) * V;
    if (base >= N) return;      // V = 4 is launched only with N % 4 == 0: a lane has all four points or none
    const unsigned XY = (unsigned)g.X * (unsigned)g.Y;
    int k = (int)((unsigned)base / XY);
    const unsigned rem = (unsigned)base - (unsigned)k * XY;
    int j = (int)(rem / (unsigned)g.X), i = (int)(rem - (unsigned)j * (unsigned)g.X);
    float sdf[V];
    int pix[V];
    bool hit[V], any = false, any_band = false;
#pragma unroll
    for (int v = 0; v < V; v++) {
        sdf[v] = 0.f;
        pix[v] = 0;
        hit[v] = project(g, c, i, j, k, depth, opacity, sdf[v], pix[v]);
        any |= hit[v];
        any_band |= hit[v] && fabsf(sdf[v]) <= c.trunc;
        if (++i == g.X) {
            i = 0;
            if (++j == g.Y) { j = 0; k++; }
        }
    }
    if (!any) return;
    // one body for both widths on hsr_lane_io.h's accessors: whatever a lane loads it stores back, changed where the point is updated
    float t[V], w[V];
    hsr_load<V>(s.tsdf + base, t);
    hsr_load<V>(s.weight + base, w);
#pragma unroll
    for (int v = 0; v < V; v++) {
        if (!hit[v]) continue;
        t[v] = running_mean(t[v], w[v], fminf(1.f, sdf[v] / c.trunc));
        w[v] = fminf(w[v] + 1.f, c.max_weight);
    }
    hsr_store<V>(s.tsdf + base, t);
    hsr_store<V>(s.weight + base, w);
    if (!any_band) return;
    if (image) {
        const long long HW = (long long)c.H * c.W;
        float cw[V];
        hsr_load<V>(s.cweight + base, cw);
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            float col[V];
            hsr_load<V>(s.color + ch * N + base, col);
#pragma unroll
            for (int v = 0; v < V; v++)
                if (hit[v] && fabsf(sdf[v]) <= c.trunc) col[v] = running_mean(col[v], cw[v], image[ch * HW + pix[v]]);
            hsr_store<V>(s.color + ch * N + base, col);
        }
#pragma unroll
        for (int v = 0; v < V; v++)
            if (hit[v] && fabsf(sdf[v]) <= c.trunc) cw[v] = fminf(cw[v] + 1.f, c.max_weight);
        hsr_store<V>(s.cweight + base, cw);
    }
    if (labels) {
        float b[V];
        int l[V];
        hsr_load<V>(s.best + base, b);
        hsr_load<V>(s.label + base, l);
#pragma unroll
        for (int v = 0; v < V; v++) {
            if (hit[v] && fabsf(sdf[v]) <= c.trunc && fabsf(sdf[v]) < b[v]) {
                b[v] = fabsf(sdf[v]);
                l[v] = (int)labels[pix[v]];
            }
        }
        hsr_store<V>(s.best + base, b);
        hsr_store<V>(s.label + base, l);
    }
}

// ---- the surface -----------------------------------------------------------------------------------------------------------------------
// the six Kuhn tetrahedra as four corner numbers (dx + 2 dy + 4 dz) of three bits each, v0 in the low bits, and their orientations
constexpr unsigned TETS[6] = {0 | 1 << 3 | 3 << 6 | 7 << 9, 0 | 1 << 3 | 5 << 6 | 7 << 9, 0 | 2 << 3 | 3 << 6 | 7 << 9,
                              0 | 2 << 3 | 6 << 6 | 7 << 9, 0 | 4 << 3 | 5 << 6 | 7 << 9, 0 | 4 << 3 | 6 << 6 | 7 << 9};
constexpr int TET_SIGN[6] = {1, -1, -1, 1, 1, -1};

__device__ __forceinline__ long long corner_lin(long long lin, int corner, int X, long long XY)
{
    return lin + (corner & 1) + ((corner >> 1) & 1) * (long long)X + ((corner >> 2) & 1) * XY;
}

// bit c: corner c of cube lin is inside; -1 where the cube is not meshed (the last layer of an axis, or a weight that is not > 0)
__device__ __forceinline__ int cube_inside(long long lin, int X, int Y, int Z, const float* __restrict__ tsdf, const float* __restrict__ weight)
{
    const long long XY = (long long)X * Y;
    const int k = (int)(lin / XY);
    const int rem = (int)(lin - k * XY);
    const int j = rem / X, i = rem - j * X;
    if (i + 1 >= X || j + 1 >= Y || k + 1 >= Z) return -1;
    int inside = 0;
    bool seen = true;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const long long p = corner_lin(lin, c, X, XY);
        seen = seen && weight[p] > 0.f;
        inside |= (tsdf[p] < 0.f ? 1 : 0) << c;
    }
    return seen ? inside : -1;
}

// the inside flags of tetrahedron `tet` (bit q: its vertex q) from the cube's
__device__ __forceinline__ int tet_mask(int inside, unsigned tet)
{
    int m = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) m |= ((inside >> ((tet >> (3 * q)) & 7u)) & 1) << q;
    return m;
}

__device__ __forceinline__ int tet_triangles(int mask)
{
    const int n = __popc((unsigned)mask);
    return n == 2 ? 2 : ((n == 1 || n == 3) ? 1 : 0);
}

// the key of the grid edge between vertices p and q (positions within the tetrahedron, any order): the corner sets of a Kuhn
// tetrahedron are nested, so the lower position is the lower endpoint and the difference an offset in {0,1}^3
__device__ __forceinline__ long long edge_key(long long lin, unsigned tet, int p, int q, int X, long long XY)
{
    const int lo = p < q ? p : q, hi = p < q ? q : p;
    const int a = (int)((tet >> (3 * lo)) & 7u), b = (int)((tet >> (3 * hi)) & 7u);
    return corner_lin(lin, a, X, XY) * 8 + (b ^ a);
}

__device__ __forceinline__ void put_triangle(long long* __restrict__ row, long long a, long long b, long long c)
{
    row[0] = a; row[1] = b; row[2] = c;
}

// the one or two triangles of a tetrahedron with inside flags `mask` (1..14) at `row`; returns their number
__device__ __forceinline__ int tet_emit(long long lin, unsigned tet, int sign, int mask, int X, long long XY, long long* __restrict__ row)
{
    const int n = __popc((unsigned)mask);
    if (n == 2) {
        const int a = __ffs(mask) - 1, b = 31 - __clz(mask);
        const int out = ~mask & 15;
        const int c = __ffs(out) - 1, d = 31 - __clz(out);
        const int inversions = (a > c) + (a > d) + (b > c) + (b > d);      // of the listing (a, b, c, d)
        const bool keep = (sign > 0) == ((inversions & 1) == 0);
        const long long ac = edge_key(lin, tet, a, c, X, XY), ad = edge_key(lin, tet, a, d, X, XY);
        const long long bd = edge_key(lin, tet, b, d, X, XY), bc = edge_key(lin, tet, b, c, X, XY);
        const long long q0 = keep ? ac : bc, q1 = keep ? ad : bd, q2 = keep ? bd : ad, q3 = keep ? bc : ac;
        const long long lo = min(min(q0, q1), min(q2, q3));
        if (lo == q0) { put_triangle(row, q0, q1, q2); put_triangle(row + 3, q0, q2, q3); }
        else if (lo == q1) { put_triangle(row, q1, q2, q3); put_triangle(row + 3, q1, q3, q0); }
        else if (lo == q2) { put_triangle(row, q2, q3, q0); put_triangle(row + 3, q2, q0, q1); }
        else { put_triangle(row, q3, q0, q1); put_triangle(row + 3, q3, q1, q2); }
        return 2;
    }
    // the lone vertex p: inside (n == 1) or outside (n == 3)
    const int lone = n == 1 ? mask : (~mask & 15);
    const int p = __ffs(lone) - 1;
    const int r0 = p == 0 ? 1 : 0, r1 = p <= 1 ? 2 : 1, r2 = p <= 2 ? 3 : 2;      // the other three, ascending
    const bool positive = (sign > 0) == ((p & 1) == 0);                             // det[r0 - p, r1 - p, r2 - p] > 0
    const bool keep = positive == (n == 1);
    const long long e0 = edge_key(lin, tet, p, r0, X, XY), e1 = edge_key(lin, tet, p, r1, X, XY), e2 = edge_key(lin, tet, p, r2, X, XY);
    put_triangle(row, e0, keep ? e1 : e2, keep ? e2 : e1);
    return 1;
}

__global__ __launch_bounds__(TB) void count_kernel(int X, int Y, int Z, long long N, const float* __restrict__ tsdf,
                                                   const float* __restrict__ weight, int* __restrict__ out_counts)
{
    const long long lin = (long long)blockIdx.x * TB + threadIdx.x;
    if (lin >= N) return;
    const int inside = cube_inside(lin, X, Y, Z, tsdf, weight);
    int n = 0;
    if (inside > 0 && inside < 255) {
#pragma unroll
        for (int t = 0; t < 6; t++) n += tet_triangles(tet_mask(inside, TETS[t]));
    }
    out_counts[lin] = n;
}

__global__ __launch_bounds__(TB) void faces_kernel(int X, int Y, int Z, long long N, const float* __restrict__ tsdf,
                                                   const float* __restrict__ weight, const long long* __restrict__ offsets, long long T,
                                                   long long* __restrict__ out_keys)
{
    const long long lin = (long long)blockIdx.x * TB + threadIdx.x;
    if (lin >= N) return;
    const int inside = cube_inside(lin, X, Y, Z, tsdf, weight);
    if (inside <= 0 || inside >= 255) return;
    int n = 0;
#pragma unroll
    for (int t = 0; t < 6; t++) n += tet_triangles(tet_mask(inside, TETS[t]));
    const long long end = offsets[lin], begin = end - n;
    if (begin < 0 || end > T) return;      // offsets that are not this volume's running sum: nothing is written out of bounds
    const long long XY = (long long)X * Y;
    long long* __restrict__ row = out_keys + 3 * begin;
#pragma unroll
    for (int t = 0; t < 6; t++) {
        const int mask = tet_mask(inside, TETS[t]);
        if (mask != 0 && mask != 15) row += 3 * tet_emit(lin, TETS[t], TET_SIGN[t], mask, X, XY, row);
    }
}

__global__ __launch_bounds__(TB) void vertices_kernel(Grid g, long long N, long long V, const long long* __restrict__ keys,
                                                      const float* __restrict__ tsdf, const float* __restrict__ color,
                                                      const float* __restrict__ cweight, const int* __restrict__ label,
                                                      float* __restrict__ out_vertices, uint8_t* __restrict__ out_rgb, int* __restrict__ out_labels)
{
    const long long v = (long long)blockIdx.x * TB + threadIdx.x;
    if (v >= V) return;
    const long long key = keys[v];
    const long long lo = key >> 3;
    const int dir = (int)(key & 7);
    if (key < 0 || lo >= N || dir == 0) return;
    const long long XY = (long long)g.X * g.Y;
    const int k = (int)(lo / XY);
    const int rem = (int)(lo - k * XY);
    const int j = rem / g.X, i = rem - j * g.X;
    const int i1 = i + (dir & 1), j1 = j + ((dir >> 1) & 1), k1 = k + ((dir >> 2) & 1);
    if (i1 >= g.X || j1 >= g.Y || k1 >= g.Z) return;
    const long long hi = corner_lin(lo, dir, g.X, XY);
    const float s0 = tsdf[lo], s1 = tsdf[hi];
    const float t = s0 / (s0 - s1);
    const float p0[3] = {g.ox + g.h * (float)i, g.oy + g.h * (float)j, g.oz + g.h * (float)k};
    const float p1[3] = {g.ox + g.h * (float)i1, g.oy + g.h * (float)j1, g.oz + g.h * (float)k1};
#pragma unroll
    for (int c = 0; c < 3; c++) out_vertices[3 * v + c] = p0[c] + t * (p1[c] - p0[c]);
    if (out_rgb) {
        const bool has0 = cweight[lo] > 0.f, has1 = cweight[hi] > 0.f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float c0 = color[c * N + lo], c1 = color[c * N + hi];
            const float mix = has0 && has1 ? c0 + t * (c1 - c0) : (has0 ? c0 : (has1 ? c1 : 0.5f));
            out_rgb[3 * v + c] = (uint8_t)hsr_colour_code(mix);
        }
    }
    if (out_labels) out_labels[v] = fabsf(s0) <= fabsf(s1) ? label[lo] : label[hi];
}

bool finite_positive(float x) { return isfinite(x) && x > 0.f; }

// the volume's size checks of every entry point; N = X * Y * Z
bool bad_grid(const char* who, int X, int Y, int Z, long long& N)
{
    N = 0;
    if (X >= 1 && Y >= 1 && Z >= 1) {
        const unsigned long long xy = (unsigned long long)X * (unsigned long long)Y;      // < 2^62
        if (xy <= 0x7fffffffull && xy * (unsigned long long)Z <= 0x7fffffffull) {
            N = (long long)(xy * (unsigned long long)Z);
            return false;
        }
    }
    hsr_set_error("%s: invalid volume X=%d Y=%d Z=%d (every side >= 1, X*Y*Z <= 2^31-1)", who, X, Y, Z);
    return true;
}

unsigned blocks_for(long long items) { return (unsigned)((items + TB - 1) / TB); }

}  // namespace

extern "C" int hsr_tsdf_integrate(int X, int Y, int Z, float ox, float oy, float oz, float h, float trunc, float max_weight, int H, int W,
                                  float fx, float fy, float cx, float cy, const float* w2c, const float* depth, const float* image,
                                  const int64_t* labels, const float* opacity, float sil_thres, float depth_max, float* tsdf, float* weight,
                                  float* color, float* cweight, float* best, int* label, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    long long N;
    if (bad_grid("tsdf_integrate", X, Y, Z, N)) return HSR_ERR_INVALID_ARGUMENT;
    if (!finite_positive(h) || !finite_positive(trunc) || !finite_positive(max_weight)) {
        hsr_set_error("tsdf_integrate: h, trunc and max_weight must be finite and positive; got %g, %g and %g", (double)h, (double)trunc,
                      (double)max_weight);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (H < 1 || W < 1 || H > HSR_TSDF_MAX_IMAGE_SIDE || W > HSR_TSDF_MAX_IMAGE_SIDE) {
        hsr_set_error("tsdf_integrate: invalid image size H=%d W=%d (1..%d)", H, W, HSR_TSDF_MAX_IMAGE_SIDE);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!w2c || !depth || !tsdf || !weight) {
        hsr_set_error("tsdf_integrate: w2c (16 floats on the host), depth, tsdf and weight are required");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if ((color == nullptr) != (cweight == nullptr) || (best == nullptr) != (label == nullptr)) {
        hsr_set_error("tsdf_integrate: color / cweight and best / label come in pairs");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if ((image && !color) || (labels && !best)) {
        hsr_set_error("tsdf_integrate: image needs color / cweight and labels need best / label");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    Grid g{X, Y, Z, ox, oy, oz, h};
    View c;
    for (int q = 0; q < 12; q++) c.m[q] = w2c[q];
    c.fx = fx; c.fy = fy; c.cx = cx; c.cy = cy;
    c.H = H; c.W = W;
    c.sil_thres = sil_thres; c.depth_max = depth_max; c.trunc = trunc; c.max_weight = max_weight;
    State s{tsdf, weight, color, cweight, best, label};
    const long long* lab = reinterpret_cast<const long long*>(labels);
    const bool wide = N % 4 == 0 && hsr_aligned(tsdf, 16) && hsr_aligned(weight, 16) && hsr_aligned(color, 16) && hsr_aligned(cweight, 16)
                      && hsr_aligned(best, 16) && hsr_aligned(label, 16);
    if (wide)
        integrate_kernel<4><<<blocks_for(N / 4), TB, 0, stream>>>(g, c, N, depth, image, lab, opacity, s);
    else
        integrate_kernel<1><<<blocks_for(N), TB, 0, stream>>>(g, c, N, depth, image, lab, opacity, s);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_tsdf_count(int X, int Y, int Z, const float* tsdf, const float* weight, int* out_counts, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    long long N;
    if (bad_grid("tsdf_count", X, Y, Z, N)) return HSR_ERR_INVALID_ARGUMENT;
    if (!tsdf || !weight || !out_counts) {
        hsr_set_error("tsdf_count: tsdf, weight and out_counts are required");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    count_kernel<<<blocks_for(N), TB, 0, stream>>>(X, Y, Z, N, tsdf, weight, out_counts);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_tsdf_faces(int X, int Y, int Z, const float* tsdf, const float* weight, const int64_t* offsets, size_t T, int64_t* out_keys,
                              void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    long long N;
    if (bad_grid("tsdf_faces", X, Y, Z, N)) return HSR_ERR_INVALID_ARGUMENT;
    if (T > (size_t)12 * (size_t)N) {
        hsr_set_error("tsdf_faces: T=%zu is more than twelve triangles per point", T);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!tsdf || !weight || !offsets || (T > 0 && !out_keys)) {
        hsr_set_error("tsdf_faces: tsdf, weight and offsets are required, and out_keys with T > 0");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (T == 0) return HSR_OK;
    faces_kernel<<<blocks_for(N), TB, 0, stream>>>(X, Y, Z, N, tsdf, weight, reinterpret_cast<const long long*>(offsets), (long long)T,
                                                   reinterpret_cast<long long*>(out_keys));
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_tsdf_vertices(int X, int Y, int Z, float ox, float oy, float oz, float h, size_t V, const int64_t* keys, const float* tsdf,
                                 const float* color, const float* cweight, const int* label, float* out_vertices, uint8_t* out_rgb,
                                 int* out_labels, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    long long N;
    if (bad_grid("tsdf_vertices", X, Y, Z, N)) return HSR_ERR_INVALID_ARGUMENT;
    if (!finite_positive(h) || V > (size_t)0x7fffffff) {
        hsr_set_error("tsdf_vertices: h must be finite and positive (got %g) and V <= 2^31-1 (got %zu)", (double)h, V);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if ((out_rgb && (!color || !cweight)) || (out_labels && !label)) {
        hsr_set_error("tsdf_vertices: out_rgb needs color and cweight, out_labels needs label");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (V > 0 && (!keys || !tsdf || !out_vertices)) {
        hsr_set_error("tsdf_vertices: keys, tsdf and out_vertices are required with V > 0");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (V == 0) return HSR_OK;
    Grid g{X, Y, Z, ox, oy, oz, h};
    vertices_kernel<<<blocks_for((long long)V), TB, 0, stream>>>(g, N, (long long)V, reinterpret_cast<const long long*>(keys), tsdf, color, cweight,
                                                                 label, out_vertices, out_rgb, out_labels);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}
