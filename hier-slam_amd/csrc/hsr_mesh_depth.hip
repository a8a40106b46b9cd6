// hsr_mesh_depth.hip — the depth image of a triangle mesh from one view (gfx950): include/recon/hsr_mesh_depth.h states the rule, and
// the rule alone defines the result; this file only divides the work.
//   setup   : setup_kernel — a face per lane: three gathered vertices into camera space, the three crosses, det, the box
//             (hsr_mesh_face.h, shared with hsr_mesh_shade.hip).  A face whose box holds at most HSR_MESH_DEPTH_SMALL_BOX pixels is rasterized right there by its lane (a ground-truth
//             mesh is a million faces of a pixel or less: a box of 9 to 16 pixels).  A larger face is appended to the list in the
//             scratch: one atomic add per wave on the counter, the order in the list does not matter.
//   sweep   : sweep_kernel — a fixed grid of SWEEP_X x SWEEP_Y workgroups, so that no host read of the count is needed: workgroup
//             (bx, by) takes the listed faces bx, bx + SWEEP_X, ... and of each face's box the 256-pixel steps by, by + SWEEP_Y, ...; it
//             recomputes the face from its vertices with setup's own function (the same bits) instead of carrying 13 floats a face
//             through memory.  A wall-sized face is therefore spread over SWEEP_Y workgroups of 256 lanes and never sits on one lane.
//   resolve : resolve_kernel — a pixel per lane: the key into out_depth and out_face.
// The pixel update: a plain load of the key, then — only when the new key is smaller — a 64-bit atomic minimum at agent scope whose
// result is unused (no return value to wait for).  The word only ever decreases, so a stale load costs a needless atomic at most.
// Every loop is bounded by what can be read here: the lane loop by HSR_MESH_DEPTH_SMALL_BOX trips, the list loop by F / SWEEP_X + 1
// and the step loop by H * W / (256 * SWEEP_Y) + 1 trips.  No workgroup waits for another; nothing spins.
// Compiled with -ffp-contract=off: every float32 operation is rounded once, in the header's order.
#include <math.h>

#include "hsr_common.h"
#include "hsr_mesh_face.h"
#include "../../include/recon/hsr_mesh_depth.h"

namespace {

constexpr int TB = 256;
constexpr int SWEEP_X = 128;      // workgroups across the list of large faces
constexpr int SWEEP_Y = 16;       // workgroups across one face's box: 2048 in all, eight per CU

typedef unsigned long long u64;

// the hit test of the header at pixel (x, y) and the pixel's minimum
__device__ __forceinline__ void test_pixel(const View& c, const Face& t, int f, int x, int y, u64* __restrict__ keys)
{
    const float rx = ((float)x - c.cx) / c.fx, ry = ((float)y - c.cy) / c.fy;
    const float wA = (rx * t.nA[0] + ry * t.nA[1]) + t.nA[2];
    const float wB = (rx * t.nB[0] + ry * t.nB[1]) + t.nB[2];
    const float wC = (rx * t.nC[0] + ry * t.nC[1]) + t.nC[2];
    const bool inside = t.det > 0.f ? (wA >= 0.f && wB >= 0.f && wC >= 0.f) : (wA <= 0.f && wB <= 0.f && wC <= 0.f);
    if (!inside) return;
    const float s = (wA + wB) + wC;
    if (s == 0.f) return;
    const float z = t.det / s;
    if (!(z < INFINITY && z >= c.near)) return;      // a NaN fails
    const u64 key = ((u64)__float_as_uint(z) << 32) | (u64)(unsigned)f;
    u64* slot = keys + (size_t)y * c.W + x;
    if (key < *slot) __hip_atomic_fetch_min(slot, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(TB) void setup_kernel(View c, int V, int F, const float* __restrict__ vertices, const int* __restrict__ faces,
                                                   u64* __restrict__ keys, int* __restrict__ large, unsigned* __restrict__ counter)
{
    const long long lane_face = (long long)blockIdx.x * TB + threadIdx.x;      // past 2^31 in the last workgroup of the largest F
    const int f = (int)lane_face;                                               // used only where lane_face < F
    Face t;
    const bool ok = lane_face < (long long)F && make_face(c, V, vertices, faces, f, t);
    const int bw = ok ? t.x1 - t.x0 + 1 : 0, n = ok ? bw * (t.y1 - t.y0 + 1) : 0;      // <= 2^28: both sides <= 16384
    const bool big = n > HSR_MESH_DEPTH_SMALL_BOX;
    // the large faces of this wave: one atomic add for all of them (every lane of the wave is here)
    const u64 votes = __ballot(big);
    if (votes != 0) {
        const int lane = threadIdx.x & 63, leader = __ffsll((long long)votes) - 1;
        unsigned base = 0;
        if (lane == leader) base = atomicAdd(counter, (unsigned)__popcll(votes));
        base = __shfl(base, leader);
        if (big) large[base + (unsigned)__popcll(votes & (((u64)1 << lane) - 1))] = f;      // < F: every face is listed at most once
    }
    if (big) return;
    for (int p = 0, x = t.x0, y = t.y0; p < n; p++) {      // n <= HSR_MESH_DEPTH_SMALL_BOX; row by row
        test_pixel(c, t, f, x, y, keys);
        if (++x > t.x1) { x = t.x0; y++; }
    }
}

__global__ __launch_bounds__(TB) void sweep_kernel(View c, int V, int F, const float* __restrict__ vertices, const int* __restrict__ faces,
                                                   u64* __restrict__ keys, const int* __restrict__ large, const unsigned* __restrict__ counter)
{
    unsigned count = *counter;      // written by setup_kernel, the launch before this one on the stream
    if (count > (unsigned)F) count = (unsigned)F;
    for (unsigned i = blockIdx.x; i < count; i += SWEEP_X) {
        const int f = large[i];
        Face t;
        if ((unsigned)f >= (unsigned)F || !make_face(c, V, vertices, faces, f, t)) continue;      // never: setup listed it
        const int bw = t.x1 - t.x0 + 1, n = bw * (t.y1 - t.y0 + 1);
        // pixel p of the box is (x0 + p % bw, y0 + p / bw); p advances by a fixed stride, so the two divisions are made once a face
        const int first = blockIdx.y * TB + threadIdx.x, dy = (SWEEP_Y * TB) / bw, dx = (SWEEP_Y * TB) % bw;
        int x = first % bw, y = first / bw;      // relative to the box's corner
        for (int p = first; p < n; p += SWEEP_Y * TB) {
            test_pixel(c, t, f, t.x0 + x, t.y0 + y, keys);
            x += dx; y += dy;
            if (x >= bw) { x -= bw; y++; }
        }
    }
}

__global__ __launch_bounds__(TB) void resolve_kernel(int N, const u64* __restrict__ keys, float* __restrict__ out_depth, int* __restrict__ out_face)
{
    const int p = blockIdx.x * TB + threadIdx.x;
    if (p >= N) return;
    const u64 key = keys[p];
    const bool hit = key != ~(u64)0;
    out_depth[p] = hit ? __uint_as_float((unsigned)(key >> 32)) : 0.f;
    out_face[p] = hit ? (int)(unsigned)key : -1;
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

struct Scratch { size_t keys, large, counter, end; };

Scratch scratch_layout(int F, int H, int W)
{
    Scratch l;
    l.keys = 0;
    l.large = align16(sizeof(u64) * (size_t)H * (size_t)W);
    l.counter = l.large + align16(sizeof(int) * (size_t)F);
    l.end = l.counter + 16;
    return l;
}

}  // namespace

extern "C" size_t hsr_mesh_depth_scratch_bytes(int F, int H, int W)
{
    if (F < 0 || H < 0 || W < 0) return 0;
    return scratch_layout(F, H, W).end;
}

extern "C" int hsr_mesh_depth(int V, int F, const float* vertices, const int* faces, int H, int W, float fx, float fy, float cx, float cy,
                              const float* w2c, float near, void* scratch, size_t scratch_bytes, float* out_depth, int* out_face, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (V < 1 || F < 0) {
        hsr_set_error("mesh_depth: invalid sizes V=%d F=%d (V >= 1, F >= 0)", V, F);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (H < 1 || W < 1 || H > HSR_MESH_MAX_IMAGE_SIDE || W > HSR_MESH_MAX_IMAGE_SIDE) {
        hsr_set_error("mesh_depth: invalid image size H=%d W=%d (1..%d)", H, W, HSR_MESH_MAX_IMAGE_SIDE);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!(isfinite(near) && near > 0.f)) {
        hsr_set_error("mesh_depth: near must be finite and positive; got %g", (double)near);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!isfinite(fx) || !isfinite(fy) || fx == 0.f || fy == 0.f || !isfinite(cx) || !isfinite(cy)) {
        hsr_set_error("mesh_depth: fx and fy must be finite and not zero, cx and cy finite; got %g, %g, %g, %g", (double)fx, (double)fy, (double)cx,
                      (double)cy);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!w2c || !out_depth || !out_face || !scratch) {
        hsr_set_error("mesh_depth: w2c (16 floats on the host), out_depth, out_face and scratch are required");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (F > 0 && (!vertices || !faces)) {
        hsr_set_error("mesh_depth: vertices and faces are required with F > 0");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const Scratch l = scratch_layout(F, H, W);
    if (scratch_bytes < l.end || (reinterpret_cast<uintptr_t>(scratch) & 15) != 0) {
        hsr_set_error("mesh_depth: the scratch must hold %zu bytes (hsr_mesh_depth_scratch_bytes) and be 16-byte aligned; %zu given", l.end,
                      scratch_bytes);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    char* base = reinterpret_cast<char*>(scratch);
    u64* keys = reinterpret_cast<u64*>(base + l.keys);
    int* large = reinterpret_cast<int*>(base + l.large);
    unsigned* counter = reinterpret_cast<unsigned*>(base + l.counter);
    const int N = H * W;      // <= 2^28
    HSR_HIP_CHECK(hipMemsetAsync(keys, 0xff, sizeof(u64) * (size_t)N, stream));
    if (F > 0) {
        View c;
        for (int q = 0; q < 12; q++) c.m[q] = w2c[q];
        c.fx = fx; c.fy = fy; c.cx = cx; c.cy = cy; c.near = near;
        c.H = H; c.W = W;
        HSR_HIP_CHECK(hipMemsetAsync(counter, 0, 16, stream));
        setup_kernel<<<(unsigned)(((long long)F + TB - 1) / TB), TB, 0, stream>>>(c, V, F, vertices, faces, keys, large, counter);
        HSR_HIP_CHECK(hipGetLastError());
        sweep_kernel<<<dim3(SWEEP_X, SWEEP_Y), TB, 0, stream>>>(c, V, F, vertices, faces, keys, large, counter);
        HSR_HIP_CHECK(hipGetLastError());
    }
    resolve_kernel<<<(unsigned)((N + TB - 1) / TB), TB, 0, stream>>>(N, keys, out_depth, out_face);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}
