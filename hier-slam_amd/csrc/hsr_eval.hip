// hsr_eval.hip — per-frame map evaluation (gfx950): PSNR / depth errors, semantic labels, per-class IoU and boundary IoU.
//
// What it replaces in the reference (utils/eval_helpers.py:1184-1630): per evaluated frame a dozen torch eager kernels for the masks,
// PSNR and depth terms, a permute + softmax + argmax per tree level followed by one masked assignment per entry of the
// label_mapping_tree dict, and a Python loop over up to ~100 classes with two host-synchronising .sum() calls, two device->host copies
// and two cv2.erode calls of d (28 at 1200x680) iterations each.  Here:
//   * metrics: ONE streaming pass over 3+3+1+1(+1) planes -> per-block partials (fp32 per thread, double across the block) -> a
//     one-block finisher in double, fixed order;
//   * labels: one thread per pixel, planar reads (coalesced per plane); the tree table is gathered from global memory (a few KB,
//     cache-resident); the leaf head keeps its [C] logits in LDS (one wave per block) and its weights in the scalar cache;
//   * boundary + counts: a pixel belongs to ONE class, so one boundary flag per pixel serves every class: the pixel is interior iff
//     the (2d+1)^2 window around it lies inside the image and holds its own label only.  Row pass: labels -> class index (int16) in
//     LDS, row-window uniformity by a scan of the LDS row; column pass: a sliding count of label changes down each column, then
//     per-block LDS histograms (integers: bit-exact in any order) flushed with 64-bit atomics.
#include "hsr_common.h"
#include "hsr_block.h"
#include "hsr_tree.h"
#include "../../include/hsr_eval.h"
#include <climits>
#include <cmath>

namespace {

constexpr int EB = 256;          // threads per block of the streaming kernels
constexpr int MET_ITEMS = 4;     // pixels per thread (metrics)
constexpr int MET_PARTS = 6;     // per-block partials: sse_r, sse_g, sse_b, |e|, sqrt(e^2), valid
constexpr int ROW_T = 256;       // row pass: pixels per block
constexpr int COL_X = 64;        // column pass: columns per block (one per lane)
constexpr int COL_R = 16;        // column pass: rows per wave strip (4 waves -> 64 rows per block)
constexpr int16_t CI_OUT = -1;   // class index of a label in no class
constexpr int16_t V_MIXED = -2;  // row window not uniform

// ---------------------------------------------------------------- frame metrics
__global__ __launch_bounds__(EB) void metrics_kernel(const float* __restrict__ im, const float* __restrict__ gt_im,
                                                     const float* __restrict__ depth, const float* __restrict__ gt_depth,
                                                     const float* __restrict__ opac, float sil_thres, int N, double* __restrict__ partials)
{
    __shared__ double s_red[EB / 64][MET_PARTS];
    float acc[MET_PARTS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = blockIdx.x * EB * MET_ITEMS + threadIdx.x, it = 0; it < MET_ITEMS; it++, i += EB) {
        if (i >= N) break;
        const float gd = gt_depth[i];
        const float valid = gd > 0.f ? 1.f : 0.f;
        const float pres = opac ? (opac[i] > sil_thres ? 1.f : 0.f) : 1.f;
        // the reference's products, in its order: im * presence * valid (presence only in the silhouette branch)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float a = opac ? (im[(size_t)c * N + i] * pres) * valid : im[(size_t)c * N + i] * valid;
            const float b = opac ? (gt_im[(size_t)c * N + i] * pres) * valid : gt_im[(size_t)c * N + i] * valid;
            const float e = a - b;
            acc[c] += e * e;
        }
        float e = depth[i] * valid - gd;
        if (opac) e = e * pres;
        acc[3] += fabsf(e) * valid;
        acc[4] += sqrtf(e * e) * valid;
        acc[5] += valid;
    }
    double accd[MET_PARTS];
#pragma unroll
    for (int k = 0; k < MET_PARTS; k++) accd[k] = (double)acc[k];
    hsr_block256_sums(accd, s_red, partials + (size_t)blockIdx.x * MET_PARTS);
}

__global__ __launch_bounds__(EB) void metrics_finish_kernel(const double* __restrict__ partials, int nblocks, int N, double* __restrict__ out3)
{
    __shared__ double s_acc[MET_PARTS][EB];
    double acc[MET_PARTS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < nblocks; b += EB)
#pragma unroll
        for (int k = 0; k < MET_PARTS; k++) acc[k] += partials[(size_t)b * MET_PARTS + k];
#pragma unroll
    for (int k = 0; k < MET_PARTS; k++) s_acc[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int o = EB / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o)
#pragma unroll
            for (int k = 0; k < MET_PARTS; k++) s_acc[k][threadIdx.x] += s_acc[k][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double psnr = 0.0;
        for (int c = 0; c < 3; c++) psnr += 20.0 * log10(1.0 / sqrt(s_acc[c][0] / (double)N));
        out3[0] = psnr / 3.0;
        out3[1] = s_acc[3][0] / s_acc[5][0];
        out3[2] = s_acc[4][0] / s_acc[5][0];
    }
}

// ---------------------------------------------------------------- labels
// argmax(softmax(.)) is hsr_tree.h's rule.  The planes are read twice (the second read hits the caches: a block's 256 pixels x n planes).
__global__ __launch_bounds__(EB) void labels_flat_kernel(const float* __restrict__ logits, int K, int N, int32_t* __restrict__ out)
{
    const int i = blockIdx.x * EB + threadIdx.x;
    if (i >= N) return;
    const float* __restrict__ x = logits + i;
    out[i] = hsr_softmax_argmax([&](int k) { return x[(size_t)k * N]; }, K);
}

__global__ __launch_bounds__(EB) void labels_tree_kernel(const float* __restrict__ logits, hsr_tree_levels lv, int N,
                                                         const int32_t* __restrict__ table, int32_t* __restrict__ out,
                                                         int32_t* __restrict__ out_levels)
{
    const int i = blockIdx.x * EB + threadIdx.x;
    if (i >= N) return;
    int idx = 0;
    for (int l = 0; l < lv.n; l++) {
        const float* __restrict__ x = logits + (size_t)lv.begin[l] * N + i;
        const int lab = hsr_softmax_argmax([&](int k) { return x[(size_t)k * N]; }, lv.size[l]);
        if (out_levels) out_levels[(size_t)l * N + i] = lab;
        idx = idx * lv.size[l] + lab;     // mixed radix, level 0 most significant (hsr_utils/evaluate.py tree_lookup_table)
    }
    out[i] = table[idx];
}

// weight [C,K] -> scratch [C][32] zero-padded, bias after it: the leaf kernel's inner loop is then a fixed 32-term FMA chain whose
// weight operands are wave-uniform scalar loads
__global__ __launch_bounds__(EB) void leaf_pack_kernel(const float* __restrict__ w, const float* __restrict__ b, int K, int C,
                                                       float* __restrict__ wp)
{
    const int t = blockIdx.x * EB + threadIdx.x;
    if (t < C * HSR_EVAL_LEAF_MAX_K) {
        const int c = t / HSR_EVAL_LEAF_MAX_K, k = t % HSR_EVAL_LEAF_MAX_K;
        wp[t] = k < K ? w[(size_t)c * K + k] : 0.f;
    } else if (t < C * (HSR_EVAL_LEAF_MAX_K + 1)) {
        const int c = t - C * HSR_EVAL_LEAF_MAX_K;
        wp[t] = b[c];
    }
}

// one wave per block; LDS: the block's C x 64 logits ([c][lane]: conflict-free), computed once, read by the passes of the label rule
__global__ __launch_bounds__(64) void labels_leaf_kernel(const float* __restrict__ sem, int K, int C, int N, const float* __restrict__ wp,
                                                         int32_t* __restrict__ out)
{
    extern __shared__ float s_z[];
    const int lane = threadIdx.x;
    const int i = blockIdx.x * 64 + lane;
    const bool live = i < N;
    float x[HSR_EVAL_LEAF_MAX_K];
#pragma unroll
    for (int k = 0; k < HSR_EVAL_LEAF_MAX_K; k++) x[k] = (live && k < K) ? sem[(size_t)k * N + i] : 0.f;
    const float* __restrict__ bias = wp + (size_t)C * HSR_EVAL_LEAF_MAX_K;
    // unrolled: the scalar loads of the weights of four classes issue together instead of one class's latency per trip
#pragma unroll 4
    for (int c = 0; c < C; c++) {
        const float* __restrict__ wc = wp + (size_t)c * HSR_EVAL_LEAF_MAX_K;
        float z = 0.f;
#pragma unroll
        for (int k = 0; k < HSR_EVAL_LEAF_MAX_K; k++) z = fmaf(wc[k], x[k], z);
        z += bias[c];
        s_z[c * 64 + lane] = z;
    }
    const int best = hsr_softmax_argmax([&](int c) { return s_z[c * 64 + lane]; }, C);
    if (live) out[i] = best;
}

// ---------------------------------------------------------------- boundary + counts
// class index of a raw label: j with ids[j] == v (binary search over the strictly ascending ids), or v itself in [0, C) when ids is
// NULL; CI_OUT for a label in no class
__device__ __forceinline__ int class_index(int v, const int32_t* __restrict__ ids, int C)
{
    if (!ids) return (v >= 0 && v < C) ? v : CI_OUT;
    int lo = 0, hi = C - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        const int t = ids[mid];
        if (t == v) return mid;
        if (t < v) lo = mid + 1; else hi = mid - 1;
    }
    return CI_OUT;
}

// grid (ceil(W / ROW_T), H, 2): z = 0 gt, 1 pred.  Writes packed[z][y][x] = ci (low 16 bits) | v (high 16 bits), v = ci when the row
// window [x-d, x+d] lies inside the image and holds class index ci only, else V_MIXED.  Distinct labels in no class share CI_OUT; that
// loses nothing: such a pixel counts for no class, and for its neighbours CI_OUT differs from every class they could have.
__global__ __launch_bounds__(ROW_T) void boundary_row_kernel(const int32_t* __restrict__ gt, const int32_t* __restrict__ pred, int H, int W,
                                                             const int32_t* __restrict__ ids, int C, int d, int32_t* __restrict__ packed)
{
    extern __shared__ int16_t s_ci[];      // ROW_T + 2d entries
    const int32_t* __restrict__ lab = blockIdx.z == 0 ? gt : pred;
    const int y = blockIdx.y, x0 = blockIdx.x * ROW_T;
    const size_t row = (size_t)y * W;
    const int span = ROW_T + 2 * d;
    for (int t = threadIdx.x; t < span; t += ROW_T) {
        const int xx = x0 - d + t;
        s_ci[t] = (xx >= 0 && xx < W) ? (int16_t)class_index(lab[row + xx], ids, C) : CI_OUT;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= W) return;
    const int ci = s_ci[threadIdx.x + d];
    bool uniform = x - d >= 0 && x + d < W;
    for (int t = threadIdx.x; uniform && t <= threadIdx.x + 2 * d; t++) uniform = s_ci[t] == ci;
    const int v = uniform ? ci : V_MIXED;
    packed[(size_t)blockIdx.z * H * W + row + x] = (int32_t)(((uint32_t)(uint16_t)v << 16) | (uint16_t)ci);
}

__device__ __forceinline__ int v_of(const int32_t* __restrict__ p, size_t at) { return p[at] >> 16; }
__device__ __forceinline__ int ci_of(int32_t packed) { return (int16_t)(packed & 0xffff); }

// Column-window state of one map for column x: the number of changes v[r] != v[r-1] for r in (y-d, y+d] inside the image.  The window
// [y-d, y+d] is interior iff it lies inside the image, that count is 0 and v[y] != V_MIXED (then every row window holds ci only).
struct ColWindow {
    int changes;
    __device__ __forceinline__ int chg(const int32_t* __restrict__ p, int r, int x, int W) const
    {
        return v_of(p, (size_t)r * W + x) != v_of(p, (size_t)(r - 1) * W + x) ? 1 : 0;
    }
};

// add `val` (count in the low 16 bits, boundary count in the high 16) to bin `ci` of an LDS histogram; all 64 lanes call it.  When
// every active lane hits one bin (the common case inside a class region) one lane adds the wave's total.
__device__ __forceinline__ void hist_add(unsigned* __restrict__ h, int ci, bool active, bool bnd)
{
    const unsigned long long act = __ballot(active);
    if (act == 0) return;
    const int leader = __ffsll((long long)act) - 1;
    const int c0 = __shfl(ci, leader, 64);
    if (__all(!active || ci == c0)) {
        const unsigned long long bb = __ballot(active && bnd);
        if ((int)(threadIdx.x & 63) == leader)
            atomicAdd(&h[c0], (unsigned)__popcll(act) + ((unsigned)__popcll(bb) << 16));
    } else if (active) {
        atomicAdd(&h[ci], 1u + (bnd ? 1u << 16 : 0u));
    }
}

// grid (ceil(W / COL_X), ceil(H / (4 * COL_R))), 256 threads: lane = column, wave = strip of COL_R rows.  LDS: 3 x C histograms
// {gt, pred, both} (at most 64 x 64 = 4096 pixels per block < 2^16: the two 16-bit halves never carry).
__global__ __launch_bounds__(EB) void boundary_count_kernel(const int32_t* __restrict__ packed, int H, int W, int C, int d,
                                                            const int32_t* __restrict__ rows, unsigned long long* __restrict__ counts)
{
    extern __shared__ unsigned s_h[];     // [3][C]
    for (int t = threadIdx.x; t < 3 * C; t += EB) s_h[t] = 0u;
    __syncthreads();
    const int32_t* __restrict__ pg = packed;
    const int32_t* __restrict__ pp = packed + (size_t)H * W;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = blockIdx.x * COL_X + lane;
    const int y0 = (blockIdx.y * 4 + wv) * COL_R;
    const bool col = x < W;
    ColWindow wg{0}, wp{0};
    // window of y0: changes over r in [max(1, y0-d+1), min(H-1, y0+d)]
    if (col) {
        const int lo = max(1, y0 - d + 1), hi = min(H - 1, y0 + d);
        for (int r = lo; r <= hi; r++) { wg.changes += wg.chg(pg, r, x, W); wp.changes += wp.chg(pp, r, x, W); }
    }
    for (int y = y0; y < y0 + COL_R; y++) {
        const bool live = col && y < H;
        int cg = CI_OUT, cp = CI_OUT;
        bool bg = true, bp = true;
        if (live) {
            if (y > y0) {
                // slide: r = y+d enters, r = y-d leaves (each only if it was / is inside [1, H-1])
                const int rin = y + d, rout = y - d;
                if (rin <= H - 1) { wg.changes += wg.chg(pg, rin, x, W); wp.changes += wp.chg(pp, rin, x, W); }
                if (rout >= 1) { wg.changes -= wg.chg(pg, rout, x, W); wp.changes -= wp.chg(pp, rout, x, W); }
            }
            const size_t at = (size_t)y * W + x;
            const int32_t qg = pg[at], qp = pp[at];
            cg = ci_of(qg);
            cp = ci_of(qp);
            const bool inside = y - d >= 0 && y + d < H;
            bg = !(inside && wg.changes == 0 && (qg >> 16) != V_MIXED);
            bp = !(inside && wp.changes == 0 && (qp >> 16) != V_MIXED);
        }
        hist_add(s_h, cg, live && cg >= 0, bg);
        hist_add(s_h + C, cp, live && cp >= 0, bp);
        hist_add(s_h + 2 * C, cg, live && cg >= 0 && cg == cp, bg && bp);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += EB) {
        const int row = rows ? rows[c] : c;
        unsigned long long* __restrict__ o = counts + (size_t)row * 6;
        const unsigned g = s_h[c], p = s_h[C + c], b = s_h[2 * C + c];
        if (g) { atomicAdd(o + 0, (unsigned long long)(g & 0xffffu)); if (g >> 16) atomicAdd(o + 3, (unsigned long long)(g >> 16)); }
        if (p) { atomicAdd(o + 1, (unsigned long long)(p & 0xffffu)); if (p >> 16) atomicAdd(o + 4, (unsigned long long)(p >> 16)); }
        if (b) { atomicAdd(o + 2, (unsigned long long)(b & 0xffffu)); if (b >> 16) atomicAdd(o + 5, (unsigned long long)(b >> 16)); }
    }
}

__global__ __launch_bounds__(EB) void miou_kernel(const long long* __restrict__ counts, int C, double* __restrict__ out2)
{
    __shared__ double s_acc[3][EB];
    double iou = 0.0, biou = 0.0, n = 0.0;
    for (int c = threadIdx.x; c < C; c += EB) {
        const long long* __restrict__ q = counts + (size_t)c * 6;
        if (q[0] + q[1] > 0) {
            iou += (double)q[2] / (double)(q[0] + q[1] - q[2]);
            biou += (double)q[5] / (double)(q[3] + q[4] - q[5]);
            n += 1.0;
        }
    }
    s_acc[0][threadIdx.x] = iou;
    s_acc[1][threadIdx.x] = biou;
    s_acc[2][threadIdx.x] = n;
    __syncthreads();
    for (int o = EB / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o)
            for (int k = 0; k < 3; k++) s_acc[k][threadIdx.x] += s_acc[k][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out2[0] = s_acc[0][0] / s_acc[2][0];   // 0 / 0 = NaN for a frame without classes, like np.mean([])
        out2[1] = s_acc[1][0] / s_acc[2][0];
    }
}

}  // namespace

// ---------------------------------------------------------------- C ABI
extern "C" size_t hsr_eval_metrics_scratch_bytes(int H, int W)
{
    if (hsr_bad_frame_size(H, W)) return 1024;
    const size_t nb = ((size_t)H * W + EB * MET_ITEMS - 1) / (EB * MET_ITEMS);
    return hsr_align256(nb * MET_PARTS * sizeof(double));
}

extern "C" int hsr_eval_frame_metrics(int H, int W, const float* im, const float* gt_im, const float* depth, const float* gt_depth,
                                      const float* final_opacity, float sil_thres, double* out3, char* scratch, size_t scratch_bytes,
                                      void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (hsr_bad_frame_size(H, W) || !im || !gt_im || !depth || !gt_depth || !out3) {
        hsr_set_error("eval_frame_metrics: invalid size H=%d W=%d or NULL im / gt_im / depth / gt_depth / out3", H, W);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    int rc = hsr_check_scratch("eval_frame_metrics", scratch, scratch_bytes, hsr_eval_metrics_scratch_bytes(H, W));
    if (rc != HSR_OK) return rc;
    const int N = H * W;
    const int nb = (N + EB * MET_ITEMS - 1) / (EB * MET_ITEMS);
    double* partials = reinterpret_cast<double*>(scratch);
    metrics_kernel<<<nb, EB, 0, stream>>>(im, gt_im, depth, gt_depth, final_opacity, sil_thres, N, partials);
    metrics_finish_kernel<<<1, EB, 0, stream>>>(partials, nb, N, out3);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_eval_labels_flat(int K, int H, int W, const float* logits, int32_t* out_labels, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (hsr_bad_frame_size(H, W) || K < 1 || !logits || !out_labels) {
        hsr_set_error("eval_labels_flat: invalid sizes K=%d H=%d W=%d or NULL logits / out_labels", K, H, W);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const int N = H * W;
    labels_flat_kernel<<<(N + EB - 1) / EB, EB, 0, stream>>>(logits, K, N, out_labels);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_eval_labels_tree(int K, int H, int W, int num_levels, const int* level_sizes, const float* logits,
                                    const int32_t* tree_table, int32_t* out_labels, int32_t* out_level_labels, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (hsr_bad_frame_size(H, W) || K < 1 || num_levels < 1 || num_levels > HSR_EVAL_MAX_LEVELS || !level_sizes || !logits || !tree_table ||
        !out_labels) {
        hsr_set_error("eval_labels_tree: invalid sizes K=%d H=%d W=%d levels=%d (1..%d) or NULL level_sizes / logits / tree_table / "
                      "out_labels", K, H, W, num_levels, HSR_EVAL_MAX_LEVELS);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    hsr_tree_levels lv;
    const hsr_tree_extent e = hsr_parse_tree_levels(num_levels, level_sizes, &lv);
    if (e.bad_level >= 0) {
        hsr_set_error("eval_labels_tree: level %d has %d classes", e.bad_level, level_sizes[e.bad_level]);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (e.sum > K || e.prod > INT_MAX) {
        hsr_set_error("eval_labels_tree: the levels need %lld of %d planes and a %lld-entry table", e.sum, K, e.prod);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const int N = H * W;
    labels_tree_kernel<<<(N + EB - 1) / EB, EB, 0, stream>>>(logits, lv, N, tree_table, out_labels, out_level_labels);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" size_t hsr_eval_leaf_scratch_bytes(int C)
{
    if (C < 1) return 256;
    return hsr_align256((size_t)C * (HSR_EVAL_LEAF_MAX_K + 1) * sizeof(float));
}

extern "C" int hsr_eval_labels_leaf(int K, int C, int H, int W, const float* sem, const float* weight, const float* bias, int32_t* out_labels,
                                    char* scratch, size_t scratch_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (hsr_bad_frame_size(H, W) || K < 1 || K > HSR_EVAL_LEAF_MAX_K || C < 1 || C > HSR_EVAL_LEAF_MAX_C || !sem || !weight || !bias || !out_labels) {
        hsr_set_error("eval_labels_leaf: invalid sizes K=%d (1..%d) C=%d (1..%d) H=%d W=%d or NULL sem / weight / bias / out_labels", K,
                      HSR_EVAL_LEAF_MAX_K, C, HSR_EVAL_LEAF_MAX_C, H, W);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    int rc = hsr_check_scratch("eval_labels_leaf", scratch, scratch_bytes, hsr_eval_leaf_scratch_bytes(C));
    if (rc != HSR_OK) return rc;
    float* wp = reinterpret_cast<float*>(scratch);
    const int np = C * (HSR_EVAL_LEAF_MAX_K + 1);
    leaf_pack_kernel<<<(np + EB - 1) / EB, EB, 0, stream>>>(weight, bias, K, C, wp);
    const int N = H * W;
    labels_leaf_kernel<<<(N + 63) / 64, 64, (size_t)C * 64 * sizeof(float), stream>>>(sem, K, C, N, wp, out_labels);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" size_t hsr_eval_iou_scratch_bytes(int H, int W)
{
    if (hsr_bad_frame_size(H, W)) return 1024;
    return hsr_align256(2 * (size_t)H * W * sizeof(int32_t));
}

extern "C" int hsr_eval_iou_counts(int H, int W, const int32_t* pred, const int32_t* gt, int C, const int32_t* sorted_ids,
                                   const int32_t* sorted_rows, int dilation, int64_t* out_counts, char* scratch, size_t scratch_bytes,
                                   void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (hsr_bad_frame_size(H, W) || C < 1 || C > HSR_EVAL_MAX_CLASSES || dilation < 1 || dilation > HSR_EVAL_MAX_DILATION || !pred || !gt ||
        !out_counts || (!sorted_ids) != (!sorted_rows)) {
        hsr_set_error("eval_iou_counts: invalid sizes H=%d W=%d C=%d (1..%d) dilation=%d (1..%d), NULL pred / gt / out_counts, or only "
                      "one of sorted_ids / sorted_rows", H, W, C, HSR_EVAL_MAX_CLASSES, dilation, HSR_EVAL_MAX_DILATION);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    int rc = hsr_check_scratch("eval_iou_counts", scratch, scratch_bytes, hsr_eval_iou_scratch_bytes(H, W));
    if (rc != HSR_OK) return rc;
    int32_t* packed = reinterpret_cast<int32_t*>(scratch);
    HSR_HIP_CHECK(hipMemsetAsync(out_counts, 0, (size_t)C * 6 * sizeof(int64_t), stream));
    boundary_row_kernel<<<dim3((W + ROW_T - 1) / ROW_T, H, 2), ROW_T, (size_t)(ROW_T + 2 * dilation) * sizeof(int16_t), stream>>>(
        gt, pred, H, W, sorted_ids, C, dilation, packed);
    boundary_count_kernel<<<dim3((W + COL_X - 1) / COL_X, (H + 4 * COL_R - 1) / (4 * COL_R)), EB, (size_t)3 * C * sizeof(unsigned), stream>>>(
        packed, H, W, C, dilation, sorted_rows, reinterpret_cast<unsigned long long*>(out_counts));
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_eval_frame_miou(int C, const int64_t* counts, double* out2, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (C < 1 || !counts || !out2) {
        hsr_set_error("eval_frame_miou: C=%d or NULL counts / out2", C);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    miou_kernel<<<1, EB, 0, stream>>>(reinterpret_cast<const long long*>(counts), C, out2);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}
