// hsr_keyframes.hip — keyframe selection by overlap for the mapping window (gfx950); include/hsr_keyframes.h has the reference lines
// (utils/keyframe_selection.py:10-96).
//   rows    : row_count_kernel (one workgroup per image row) -> row_scan_kernel (one workgroup: exclusive prefix, total);
//   sample  : sample_kernel — one wave per rank: binary search of the row prefix, then ballot + popcount along the row; back-projection;
//             dedupe_kernel — one workgroup: the rounding keys of all n points in LDS, all pairs, order-preserving compaction;
//   overlap : overlap_kernel — one workgroup per keyframe, integer count reduced over its waves.
// Small and latency-bound: 5 launches per selection in place of ~17 per keyframe.  Compiled with -ffp-contract=off: the chains decide
// integers (the key equality, the five tests), so they are evaluated in the order written, without FMA contraction.
#include "hsr_common.h"
#include "hsr_block.h"
#include "../../include/hsr_keyframes.h"

namespace {

constexpr int KB = 256;

__global__ __launch_bounds__(KB) void row_count_kernel(int W, const float* __restrict__ depth, int* __restrict__ row_prefix)
{
    __shared__ int s_w[KB / 64];
    const float* row = depth + (size_t)blockIdx.x * W;
    int local = 0;
    for (int x = threadIdx.x; x < W; x += KB) local += row[x] > 0.f ? 1 : 0;
    const int total = hsr_block256_isum(local, s_w);
    if (threadIdx.x == 0) row_prefix[blockIdx.x] = total;
}

// in place: counts[0, H) -> exclusive prefix, total -> counts[H]
__global__ __launch_bounds__(1024) void row_scan_kernel(int H, int* __restrict__ counts)
{
    __shared__ int s_w[17];
    const int total = hsr_block1024_exclusive_scan(H, counts, s_w);
    if (threadIdx.x == 0) counts[H] = total;
}

// one wave per rank; r and everything derived from it is wave-uniform, so the loops do not diverge
__global__ __launch_bounds__(KB) void sample_kernel(int H, int W, const float* __restrict__ depth, const int* __restrict__ row_prefix, int n,
                                                    const int64_t* __restrict__ ranks, hsr_pinhole f, const float* __restrict__ c2w,
                                                    float* __restrict__ raw_pts, int* __restrict__ out_pixels)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (KB / 64) + (threadIdx.x >> 6);
    if (i >= n) return;
    const int64_t r = ranks[i];
    if (r < 0 || r >= (int64_t)row_prefix[H]) {   // not a rank torch.randint(n_valid, ...) draws: an origin point, which the rule removes
        if (lane == 0) {
            out_pixels[2 * i] = -1; out_pixels[2 * i + 1] = -1;
            raw_pts[3 * i] = 0.f; raw_pts[3 * i + 1] = 0.f; raw_pts[3 * i + 2] = 0.f;
        }
        return;
    }
    // the row: first index in [1, H] whose prefix exceeds r, minus one (rows without a valid pixel are stepped over)
    int lo = 1, hi = H;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)row_prefix[mid] > r) hi = mid; else lo = mid + 1;
    }
    const int row = lo - 1;
    int k = (int)(r - row_prefix[row]);
    const float* drow = depth + (size_t)row * W;
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        const float z = x < W ? drow[x] : 0.f;
        const bool v = z > 0.f;
        const unsigned long long b = __ballot(v);
        const int c = __popcll(b);
        if (k >= c) { k -= c; continue; }
        if (v && __popcll(b & ((1ull << lane) - 1ull)) == k) {
            hsr_backproject((float)x, (float)row, z, f, c2w, raw_pts + 3 * i);   // get_pointcloud (:17-25)
            out_pixels[2 * i] = row; out_pixels[2 * i + 1] = x;
        }
        return;
    }
    if (lane == 0) {   // the row holds fewer valid pixels than its prefix says: depth changed since valid_rows; removed like a bad rank
        out_pixels[2 * i] = -1; out_pixels[2 * i + 1] = -1;
        raw_pts[3 * i] = 0.f; raw_pts[3 * i + 1] = 0.f; raw_pts[3 * i + 2] = 0.f;
    }
}

// torch.round(x, decimals=4) as torch's device kernel writes it (nearbyint(x * 10^4) / 10^4 in fp32), then abs (:28)
__device__ __forceinline__ float round_key(float x) { return fabsf(nearbyintf(x * 10000.0f) / 10000.0f); }

__global__ __launch_bounds__(KB) void round_keys_kernel(int n, const float* __restrict__ vals, float* __restrict__ out)
{
    const int i = blockIdx.x * KB + threadIdx.x;
    if (i < n) out[i] = round_key(vals[i]);
}

// :28-35 for n <= HSR_KF_MAX_POINTS points in one workgroup.  unique(dim=0) with counts > 1 over [keys; (0,0,0)] marks every point whose
// key is zero or occurs twice; here: all pairs over the keys in LDS (every lane of a wave reads the same j: an LDS broadcast).
__global__ __launch_bounds__(1024) void dedupe_kernel(int n, const float* __restrict__ raw_pts, float* __restrict__ out_pts,
                                                      uint8_t* __restrict__ out_keep, int* __restrict__ out_count)
{
    __shared__ float s_kx[HSR_KF_MAX_POINTS], s_ky[HSR_KF_MAX_POINTS], s_kz[HSR_KF_MAX_POINTS];
    __shared__ unsigned s_w[16];
    for (int i = threadIdx.x; i < n; i += 1024) {
        s_kx[i] = round_key(raw_pts[3 * i]); s_ky[i] = round_key(raw_pts[3 * i + 1]); s_kz[i] = round_key(raw_pts[3 * i + 2]);
    }
    __syncthreads();
    int run = 0;   // survivors before this pass: the same in every thread
    for (int base = 0; base < n; base += 1024) {
        const int i = base + threadIdx.x;
        bool keep = false;
        if (i < n) {
            const float a = s_kx[i], b = s_ky[i], c = s_kz[i];
            bool rem = (a == 0.f && b == 0.f && c == 0.f);
            for (int j = 0; j < n; j++) rem = rem || (j != i && s_kx[j] == a && s_ky[j] == b && s_kz[j] == c);
            keep = !rem;
            out_keep[i] = keep ? 1 : 0;
        }
        unsigned total;
        const int pos = run + (int)hsr_block_rank<16>(keep, s_w, &total);
        if (keep) { out_pts[3 * pos] = raw_pts[3 * i]; out_pts[3 * pos + 1] = raw_pts[3 * i + 1]; out_pts[3 * pos + 2] = raw_pts[3 * i + 2]; }
        run += (int)total;
        __syncthreads();   // s_w has been read by every wave before the next pass writes it
    }
    if (threadIdx.x == 0) *out_count = run;
}

struct Proj { float umax, vmax, edge; };

// one workgroup per keyframe.  Every point is read once per keyframe and all keyframes read the same <= 48 KB, which stays in L2: staging
// it in LDS would copy it once per workgroup for a single use.
__global__ __launch_bounds__(KB) void overlap_kernel(int n_cap, const int* __restrict__ n_dev, const float* __restrict__ pts,
                                                     const float* __restrict__ w2c, const float* __restrict__ intr, Proj p,
                                                     int* __restrict__ out_counts)
{
    __shared__ int s_w[KB / 64];
    int n = n_cap;
    if (n_dev) { n = *n_dev; n = n < 0 ? 0 : (n > n_cap ? n_cap : n); }
    const float* m = w2c + 16 * (size_t)blockIdx.x;
    float w[12], k[9];
#pragma unroll
    for (int q = 0; q < 12; q++) w[q] = m[q];
#pragma unroll
    for (int q = 0; q < 9; q++) k[q] = intr[q];
    int local = 0;
    for (int i = threadIdx.x; i < n; i += KB) {
        const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        const float t0 = ((w[0] * x + w[1] * y) + w[2] * z) + w[3] * 1.0f;      // :69-70
        const float t1 = ((w[4] * x + w[5] * y) + w[6] * z) + w[7] * 1.0f;
        const float t2 = ((w[8] * x + w[9] * y) + w[10] * z) + w[11] * 1.0f;
        const float p0 = (k[0] * t0 + k[1] * t1) + k[2] * t2;             // :72
        const float p1 = (k[3] * t0 + k[4] * t1) + k[5] * t2;
        const float p2 = (k[6] * t0 + k[7] * t1) + k[8] * t2;
        const float zz = p2 + 1e-5f;                                            // :74
        const float u = p0 / zz, v = p1 / zz;                                   // :75-76
        local += (u < p.umax && u > p.edge && v < p.vmax && v > p.edge && zz > 0.f) ? 1 : 0;   // :79-81
    }
    const int total = hsr_block256_isum(local, s_w);
    if (threadIdx.x == 0) out_counts[blockIdx.x] = total;
}

}  // namespace

extern "C" int hsr_kf_valid_rows(int H, int W, const float* depth, int32_t* row_prefix, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (hsr_bad_frame_size(H, W) || !depth || !row_prefix) {
        hsr_set_error("kf_valid_rows: invalid sizes H=%d W=%d or NULL depth/row_prefix", H, W);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    row_count_kernel<<<H, KB, 0, stream>>>(W, depth, row_prefix);
    row_scan_kernel<<<1, 1024, 0, stream>>>(H, row_prefix);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" size_t hsr_kf_sample_scratch_bytes(int n)
{
    return (size_t)(n > 0 ? n : 1) * 3 * sizeof(float) + 256;
}

extern "C" int hsr_kf_sample_points(int H, int W, const float* depth, const int32_t* row_prefix, int n, const int64_t* ranks, float fx,
                                    float fy, float cx, float cy, const float* c2w, float* out_pts, int32_t* out_pixels,
                                    uint8_t* out_keep, int32_t* out_count, char* scratch, size_t scratch_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (hsr_bad_frame_size(H, W) || n < 1 || n > HSR_KF_MAX_POINTS) {
        hsr_set_error("kf_sample_points: invalid sizes H=%d W=%d n=%d (1 <= n <= %d)", H, W, n, HSR_KF_MAX_POINTS);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!depth || !row_prefix || !ranks || !c2w || !out_pts || !out_pixels || !out_keep || !out_count) {
        hsr_set_error("kf_sample_points: NULL depth/row_prefix/ranks/c2w/out_pts/out_pixels/out_keep/out_count");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (int rc = hsr_check_scratch("kf_sample_points", scratch, scratch_bytes, hsr_kf_sample_scratch_bytes(n))) return rc;
    float* raw = reinterpret_cast<float*>(scratch);
    hsr_pinhole f{fx, fy, cx, cy};
    const int per = KB / 64;
    sample_kernel<<<(n + per - 1) / per, KB, 0, stream>>>(H, W, depth, row_prefix, n, ranks, f, c2w, raw, out_pixels);
    dedupe_kernel<<<1, 1024, 0, stream>>>(n, raw, out_pts, out_keep, out_count);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_kf_round_keys(int n, const float* vals, float* out_keys, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || (n > 0 && (!vals || !out_keys))) {
        hsr_set_error("kf_round_keys: invalid arguments (n=%d)", n);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return HSR_OK;
    round_keys_kernel<<<(n + KB - 1) / KB, KB, 0, stream>>>(n, vals, out_keys);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_kf_overlap_counts(int n_pts, const int32_t* n_pts_dev, const float* pts, int n_kf, const float* w2c, const float* intr,
                                     int W, int H, int edge, int32_t* out_counts, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n_pts < 0 || n_kf < 0 || W < 1 || H < 1 || (n_kf > 0 && (!w2c || !intr || !out_counts)) || (n_kf > 0 && n_pts > 0 && !pts)) {
        hsr_set_error("kf_overlap_counts: invalid arguments (n_pts=%d n_kf=%d W=%d H=%d) or NULL pts/w2c/intr/out_counts", n_pts, n_kf, W, H);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (n_kf == 0) return HSR_OK;
    if (n_pts == 0) {
        HSR_HIP_CHECK(hipMemsetAsync(out_counts, 0, (size_t)n_kf * sizeof(int32_t), stream));
        return HSR_OK;
    }
    Proj p;
    p.umax = (float)(W - edge); p.vmax = (float)(H - edge); p.edge = (float)edge;
    overlap_kernel<<<n_kf, KB, 0, stream>>>(n_pts, n_pts_dev, pts, w2c, intr, p, out_counts);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}
