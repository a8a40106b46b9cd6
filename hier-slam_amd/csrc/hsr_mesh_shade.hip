// hsr_mesh_shade.hip — pictures of a triangle mesh from one view (gfx950), DESIGN.md §7 row 20: include/shade/hsr_mesh_shade.h states
// both rules operation by operation, and the rules alone define the results; this file only divides the work.
//   normals : face_normal_kernel — a face per lane: three gathered vertices, one cross in float32, three 64-bit fixed-point words, nine
//             integer atomic adds at agent scope whose results are unused (nothing to wait for).  vertex_normal_kernel — a vertex per
//             lane: the three sums to float64, one sqrt, three divisions.  Integer sums: no order of arrival can change a bit.
//   shade   : shade_kernel<P> — P = 4: a lane takes 4 consecutive pixels of the flat index, whatever W is, and writes three dwords per
//             picture; the last H * W % 4 pixels of the image go out byte by byte from the same registers.  P = 1: a pixel per lane and
//             three byte stores, for calls with an out off 4 bytes.  Per pixel the face's terms are recomputed from its three vertices by
//             hsr_mesh_face.h (the depth kernel's own functions: the same bits) — 9 gathered floats instead of 13 carried through
//             memory — and the weights, hit point, view vector and flat normal are computed ONCE for all jobs; the job loop is unrolled
//             over HSR_SHADE_MAX_JOBS with wave-uniform guards, so every job struct is read from the kernel arguments with a constant
//             index (scalar loads, no scratch) and the packed bytes stay in registers.  A smooth normal is recomputed only when a job's
//             normals pointer differs from the previous job's.  Gather-bound: neighbouring pixels mostly share a face, so the gathers
//             of a wave hit a handful of lines; nothing is staged in LDS.
// Every index is checked before use: the pixel's face against F, its vertices against V (face_terms), a label against n; a SCALAR
// index is 0..255 by the clamp and n == 256 is required by the entry point.
// Compiled with -ffp-contract=off: every operation is rounded once, in the header's order.
#include <math.h>

#include "hsr_common.h"
#include "hsr_lane_io.h"
#include "hsr_mesh_face.h"
#include "../../include/recon/hsr_mesh_depth.h"
#include "../../include/shade/hsr_mesh_shade.h"

namespace {

constexpr int TB = 256;
constexpr double FIX = 1099511627776.0;      // 2^40
constexpr float NORMAL_LIMIT = 65536.f;      // 2^16

typedef unsigned long long u64;

// ---- vertex normals ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void face_normal_kernel(int V, int F, const float* __restrict__ vertices, const int* __restrict__ faces,
                                                         u64* __restrict__ sums)
{
    const long long lane_face = (long long)blockIdx.x * TB + threadIdx.x;
    if (lane_face >= (long long)F) return;
    const size_t f = (size_t)lane_face;
    const int idx[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    if (!((unsigned)idx[0] < (unsigned)V && (unsigned)idx[1] < (unsigned)V && (unsigned)idx[2] < (unsigned)V)) return;
    const float* a = vertices + 3 * (size_t)idx[0];
    const float* b = vertices + 3 * (size_t)idx[1];
    const float* d = vertices + 3 * (size_t)idx[2];
    const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {d[0] - a[0], d[1] - a[1], d[2] - a[2]};
    float c[3];
    cross(e1, e2, c);
    if (!(fabsf(c[0]) < NORMAL_LIMIT && fabsf(c[1]) < NORMAL_LIMIT && fabsf(c[2]) < NORMAL_LIMIT)) return;      // a NaN fails
    u64 q[3];
#pragma unroll
    for (int k = 0; k < 3; k++) q[k] = (u64)llrint((double)c[k] * FIX);      // |q| < 2^56; unsigned: wrap-around is defined
#pragma unroll
    for (int corner = 0; corner < 3; corner++)
#pragma unroll
        for (int k = 0; k < 3; k++)
            __hip_atomic_fetch_add(sums + 3 * (size_t)idx[corner] + k, q[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(TB) void vertex_normal_kernel(int V, const u64* __restrict__ sums, float* __restrict__ out)
{
    const long long lane_vertex = (long long)blockIdx.x * TB + threadIdx.x;
    if (lane_vertex >= (long long)V) return;
    const size_t v = (size_t)lane_vertex;
    double d[3];
#pragma unroll
    for (int k = 0; k < 3; k++) d[k] = (double)(long long)sums[3 * v + k] * (1.0 / FIX);      // 2^-40: exact
    const double len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) out[3 * v + k] = len == 0.0 ? 0.f : (float)(d[k] / len);
}

// ---- the pictures --------------------------------------------------------------------------------------------------------------------
struct Jobs {
    hsr_shade_job j[HSR_SHADE_MAX_JOBS];
};

struct Camera {
    float m[12];      // rows 0..2 of the world-to-camera matrix
    float fx, fy, cx, cy;
    int W;
};

// what all jobs of a pixel share
struct Pixel {
    bool hit;
    int idx[3];
    float b[3], p[3], v[3], nf[3];
};

__device__ __forceinline__ float dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// n / |n| into out; false when |n| is 0 or not finite
__device__ __forceinline__ bool unit3(const float* n, float* out)
{
    const float len = sqrtf(dot3(n, n));
    if (!(len > 0.f && len < INFINITY)) return false;      // a NaN fails
    out[0] = n[0] / len; out[1] = n[1] / len; out[2] = n[2] / len;
    return true;
}

__device__ __forceinline__ void setup_pixel(const Camera& c, int V, int F, const float* __restrict__ vertices, const int* __restrict__ faces,
                                            const int* __restrict__ face_image, long long i, Pixel& px)
{
    px.hit = false;
    const int f = face_image[i];
    if ((unsigned)f >= (unsigned)F) return;
    Face t;
    float A[3], B[3], C[3];
    if (!face_terms(c.m, V, vertices, faces, f, px.idx, A, B, C, t)) return;
    const int y = (int)(i / c.W), x = (int)(i - (long long)y * c.W);
    const float rx = ((float)x - c.cx) / c.fx, ry = ((float)y - c.cy) / c.fy;
    const float wA = (rx * t.nA[0] + ry * t.nA[1]) + t.nA[2];
    const float wB = (rx * t.nB[0] + ry * t.nB[1]) + t.nB[2];
    const float wC = (rx * t.nC[0] + ry * t.nC[1]) + t.nC[2];
    const float s = (wA + wB) + wC;
    if (s == 0.f) return;
    px.b[0] = wA / s; px.b[1] = wB / s; px.b[2] = wC / s;
    const float z = t.det / s;
    if (!(z > 0.f && z < INFINITY)) return;      // a NaN fails
    px.p[0] = z * rx; px.p[1] = z * ry; px.p[2] = z;
    const float l = sqrtf(dot3(px.p, px.p));
    px.v[0] = -px.p[0] / l; px.v[1] = -px.p[1] / l; px.v[2] = -px.p[2] / l;
    const float e1[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, e2[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
    float g[3];
    cross(e1, e2, g);
    if (!unit3(g, px.nf)) { px.nf[0] = 0.f; px.nf[1] = 0.f; px.nf[2] = -1.f; }
    px.hit = true;
}

// the shading normal of the header for `normals` (NULL: flat), turned towards the camera
__device__ __forceinline__ void shading_normal(const Camera& c, const Pixel& px, const float* __restrict__ normals, float* n)
{
    n[0] = px.nf[0]; n[1] = px.nf[1]; n[2] = px.nf[2];
    if (normals) {
        float r[3][3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float* w = normals + 3 * (size_t)px.idx[k];      // idx < V: face_terms checked it
            const float nx = w[0], ny = w[1], nz = w[2];
            r[k][0] = (c.m[0] * nx + c.m[1] * ny) + c.m[2] * nz;
            r[k][1] = (c.m[4] * nx + c.m[5] * ny) + c.m[6] * nz;
            r[k][2] = (c.m[8] * nx + c.m[9] * ny) + c.m[10] * nz;
        }
        float t[3], u[3];
#pragma unroll
        for (int k = 0; k < 3; k++) t[k] = (px.b[0] * r[0][k] + px.b[1] * r[1][k]) + px.b[2] * r[2][k];
        if (unit3(t, u)) { n[0] = u[0]; n[1] = u[1]; n[2] = u[2]; }
    }
    if (dot3(n, px.p) > 0.f) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
}

__device__ __forceinline__ unsigned lit_byte(unsigned byte, bool lit, float shade)
{
    return lit ? (unsigned)hsr_colour_code((float)byte / 255.0f * shade) : byte;
}

// the three bytes of job's picture at a pixel that hit, packed R | G << 8 | B << 16
__device__ __forceinline__ unsigned job_colour(const hsr_shade_job& job, const Pixel& px, const float* n)
{
    const float shade = job.ambient + (1.0f - job.ambient) * fabsf(dot3(n, px.v));
    const bool lit = job.lit != 0;
    unsigned r, g, b;
    if (job.kind == HSR_SHADE_SHADED) {
        r = (unsigned)hsr_colour_code(job.albedo[0] * shade);
        g = (unsigned)hsr_colour_code(job.albedo[1] * shade);
        b = (unsigned)hsr_colour_code(job.albedo[2] * shade);
    } else if (job.kind == HSR_SHADE_COLOUR) {
        const uint8_t* __restrict__ col = static_cast<const uint8_t*>(job.attr);
        const uint8_t* cA = col + 3 * (size_t)px.idx[0];
        const uint8_t* cB = col + 3 * (size_t)px.idx[1];
        const uint8_t* cC = col + 3 * (size_t)px.idx[2];
        unsigned out[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            float t = ((px.b[0] * (float)cA[k] + px.b[1] * (float)cB[k]) + px.b[2] * (float)cC[k]) / 255.0f;
            if (lit) t = t * shade;
            out[k] = (unsigned)hsr_colour_code(t);
        }
        r = out[0]; g = out[1]; b = out[2];
    } else if (job.kind == HSR_SHADE_NORMALS) {
        r = (unsigned)hsr_colour_code(n[0] * 0.5f + 0.5f);
        g = (unsigned)hsr_colour_code(-n[1] * 0.5f + 0.5f);
        b = (unsigned)hsr_colour_code(-n[2] * 0.5f + 0.5f);
    } else {
        int row;
        bool ok = true;
        if (job.kind == HSR_SHADE_LABELS) {
            int k = 0;
            if (px.b[1] > px.b[k]) k = 1;
            if (px.b[2] > px.b[k]) k = 2;
            row = static_cast<const int*>(job.attr)[k == 0 ? px.idx[0] : (k == 1 ? px.idx[1] : px.idx[2])];
            ok = row >= 0 && row < job.n;
        } else {      // HSR_SHADE_SCALAR
            const float* __restrict__ val = static_cast<const float*>(job.attr);
            const float t = (px.b[0] * val[px.idx[0]] + px.b[1] * val[px.idx[1]]) + px.b[2] * val[px.idx[2]];
            row = (int)(hsr_clamp01((t - job.lo) / (job.hi - job.lo)) * 255.0f);      // 0..255, and n == 256
        }
        r = g = b = 0;
        if (ok) {
            const uint8_t* __restrict__ entry = job.table + 3 * (size_t)row;
            r = lit_byte(entry[0], lit, shade);
            g = lit_byte(entry[1], lit, shade);
            b = lit_byte(entry[2], lit, shade);
        }
    }
    return r | g << 8 | b << 16;
}

template <int P>
__global__ __launch_bounds__(TB) void shade_kernel(Camera c, int V, int F, const float* __restrict__ vertices, const int* __restrict__ faces,
                                                   const int* __restrict__ face_image, Jobs jobs, int n_jobs, long long N)
{
    const long long i0 = ((long long)blockIdx.x * TB + threadIdx.x) * P;
    if (i0 >= N) return;
    const int count = N - i0 < P ? (int)(N - i0) : P;      // < P only in the image's last lane
    unsigned w[HSR_SHADE_MAX_JOBS][3] = {};                // 12 bytes a picture: pixel q's R, G, B are bytes 3q, 3q + 1, 3q + 2
#pragma unroll
    for (int q = 0; q < P; q++) {
        if (q >= count) continue;
        Pixel px;
        setup_pixel(c, V, F, vertices, faces, face_image, i0 + q, px);
        const float* have = nullptr;
        bool first = true;
        float n[3] = {0.f, 0.f, -1.f};
#pragma unroll
        for (int k = 0; k < HSR_SHADE_MAX_JOBS; k++) {
            if (k >= n_jobs) continue;      // wave-uniform
            const hsr_shade_job& job = jobs.j[k];
            unsigned rgb;
            if (px.hit) {
                if (first || job.normals != have) {      // wave-uniform: the same normals as the job before give the same normal
                    shading_normal(c, px, job.normals, n);
                    have = job.normals;
                    first = false;
                }
                rgb = job_colour(job, px, n);
            } else {
                rgb = (unsigned)job.background[0] | (unsigned)job.background[1] << 8 | (unsigned)job.background[2] << 16;
            }
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                const int byte = 3 * q + ch;
                w[k][byte >> 2] |= ((rgb >> (8 * ch)) & 0xffu) << (8 * (byte & 3));
            }
        }
    }
#pragma unroll
    for (int k = 0; k < HSR_SHADE_MAX_JOBS; k++) {
        if (k >= n_jobs) continue;
        uint8_t* __restrict__ out = jobs.j[k].out + 3 * (size_t)i0;      // i0 + count <= N: inside [H,W,3]
        if (P == 4 && count == 4) {
            unsigned* __restrict__ o = reinterpret_cast<unsigned*>(out);      // out is 4-byte aligned and 3 * i0 a multiple of 4
            o[0] = w[k][0]; o[1] = w[k][1]; o[2] = w[k][2];
        } else {
#pragma unroll
            for (int byte = 0; byte < 3 * P; byte++)
                if (byte < 3 * count) out[byte] = (uint8_t)(w[k][byte >> 2] >> (8 * (byte & 3)));
        }
    }
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

extern "C" size_t hsr_mesh_normals_scratch_bytes(int V)
{
    if (V < 0) return 0;
    return align16(24 * (size_t)V);
}

extern "C" int hsr_mesh_normals(int V, int F, const float* vertices, const int* faces, void* scratch, size_t scratch_bytes, float* out_normals,
                                void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (V < 1 || F < 0) {
        hsr_set_error("mesh_shade: normals: invalid sizes V=%d F=%d (V >= 1, F >= 0)", V, F);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!vertices || !scratch || !out_normals) {
        hsr_set_error("mesh_shade: normals: vertices, scratch and out_normals are required");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (F > 0 && !faces) {
        hsr_set_error("mesh_shade: normals: faces are required with F > 0");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const size_t need = hsr_mesh_normals_scratch_bytes(V);
    if (scratch_bytes < need || !hsr_aligned(scratch, 16)) {
        hsr_set_error("mesh_shade: normals: the scratch must hold %zu bytes (hsr_mesh_normals_scratch_bytes) and be 16-byte aligned; %zu given",
                      need, scratch_bytes);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    u64* sums = reinterpret_cast<u64*>(scratch);
    HSR_HIP_CHECK(hipMemsetAsync(sums, 0, 24 * (size_t)V, stream));
    if (F > 0) {
        face_normal_kernel<<<(unsigned)(((long long)F + TB - 1) / TB), TB, 0, stream>>>(V, F, vertices, faces, sums);
        HSR_HIP_CHECK(hipGetLastError());
    }
    vertex_normal_kernel<<<(unsigned)(((long long)V + TB - 1) / TB), TB, 0, stream>>>(V, sums, out_normals);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_mesh_shade(int V, int F, const float* vertices, const int* faces, int H, int W, float fx, float fy, float cx, float cy,
                              const float* w2c, const int* face_image, int n_jobs, const hsr_shade_job* jobs, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (V < 1 || F < 0) {
        hsr_set_error("mesh_shade: invalid sizes V=%d F=%d (V >= 1, F >= 0)", V, F);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (H < 1 || W < 1 || H > HSR_MESH_MAX_IMAGE_SIDE || W > HSR_MESH_MAX_IMAGE_SIDE) {
        hsr_set_error("mesh_shade: invalid image size H=%d W=%d (1..%d)", H, W, HSR_MESH_MAX_IMAGE_SIDE);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!isfinite(fx) || !isfinite(fy) || fx == 0.f || fy == 0.f || !isfinite(cx) || !isfinite(cy)) {
        hsr_set_error("mesh_shade: fx and fy must be finite and not zero, cx and cy finite; got %g, %g, %g, %g", (double)fx, (double)fy, (double)cx,
                      (double)cy);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!w2c || !face_image) {
        hsr_set_error("mesh_shade: w2c (16 floats on the host) and face_image are required");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (F > 0 && (!vertices || !faces)) {
        hsr_set_error("mesh_shade: vertices and faces are required with F > 0");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (n_jobs < 1 || n_jobs > HSR_SHADE_MAX_JOBS || !jobs) {
        hsr_set_error("mesh_shade: n_jobs must be 1..%d with a host array of that many jobs; got %d", HSR_SHADE_MAX_JOBS, n_jobs);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    Jobs kj{};
    bool vec = true;
    for (int k = 0; k < n_jobs; k++) {
        const hsr_shade_job& j = jobs[k];
        if (j.kind < HSR_SHADE_SHADED || j.kind > HSR_SHADE_SCALAR) {
            hsr_set_error("mesh_shade: job %d: unknown kind %d", k, j.kind);
            return HSR_ERR_INVALID_ARGUMENT;
        }
        const bool attr = j.kind == HSR_SHADE_COLOUR || j.kind == HSR_SHADE_LABELS || j.kind == HSR_SHADE_SCALAR;
        const bool table = j.kind == HSR_SHADE_LABELS || j.kind == HSR_SHADE_SCALAR;
        if (!j.out || (attr && !j.attr) || (table && !j.table)) {
            hsr_set_error("mesh_shade: job %d (kind %d): NULL out, attr or table", k, j.kind);
            return HSR_ERR_INVALID_ARGUMENT;
        }
        if ((j.kind == HSR_SHADE_SCALAR && j.n != 256) || (j.kind == HSR_SHADE_LABELS && j.n < 1)) {
            hsr_set_error("mesh_shade: job %d (kind %d): a table of %d rows; SCALAR takes 256, LABELS at least 1", k, j.kind, j.n);
            return HSR_ERR_INVALID_ARGUMENT;
        }
        if (j.kind == HSR_SHADE_SCALAR) {
            const float range = j.hi - j.lo;
            if (!isfinite(range) || !(range > 0.f)) {
                hsr_set_error("mesh_shade: job %d: hi - lo must be finite and positive; got lo %g hi %g", k, (double)j.lo, (double)j.hi);
                return HSR_ERR_INVALID_ARGUMENT;
            }
        }
        if (!(j.ambient >= 0.f && j.ambient <= 1.f)) {      // a NaN fails
            hsr_set_error("mesh_shade: job %d: ambient must be in [0, 1]; got %g", k, (double)j.ambient);
            return HSR_ERR_INVALID_ARGUMENT;
        }
        vec = vec && hsr_aligned(j.out, 4);
        kj.j[k] = j;
    }
    Camera c;
    for (int q = 0; q < 12; q++) c.m[q] = w2c[q];
    c.fx = fx; c.fy = fy; c.cx = cx; c.cy = cy;
    c.W = W;
    const long long N = (long long)H * W;      // <= 2^28
    if (vec)
        shade_kernel<4><<<(unsigned)(((N + 3) / 4 + TB - 1) / TB), TB, 0, stream>>>(c, V, F, vertices, faces, face_image, kj, n_jobs, N);
    else
        shade_kernel<1><<<(unsigned)((N + TB - 1) / TB), TB, 0, stream>>>(c, V, F, vertices, faces, face_image, kj, n_jobs, N);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}
