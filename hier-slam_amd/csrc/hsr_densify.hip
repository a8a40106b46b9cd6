// hsr_densify.hip — silhouette densification of one mapped frame on device (gfx950), SURVEY.md §8(f) rank 3.
// See include/hsr_densify.h for the reference lines (scripts/hierslam.py:1264-1305, :144-194, :1157).
//   median : 4 x (select_hist_kernel -> select_pick_kernel): 8-bit radix select, most significant byte first, of the rank
//            (N-1)/2 element of depth_error's bit patterns (torch.median = lower median); the first histogram pass also counts
//            the NaN errors, and with one or more of them the last pick leaves NaN (torch.median's rule), which empties the
//            depth part of the mask;
//   mask   : mask_count_kernel — the non-presence mask + one count per 256-pixel block;
//   scan   : scan_counts_kernel — one workgroup, exclusive scan of the block counts, total -> out_count;
//   emit   : emit_points_kernel — order-preserving compaction (block offset + wave ballot rank), back-projection, colours,
//            log-scales.  Compiled with -ffp-contract=off: the emitted means are what the rasterizer will bin next.
#include "hsr_common.h"
#include "hsr_block.h"
#include "../../include/hsr_densify.h"

namespace {

constexpr int DB = 256;

// device scratch: bits fixed so far, their mask, remaining rank, the number of NaN errors (torch.median: any NaN -> NaN)
struct SelectState { unsigned prefix, mask, rank, nan; };

__global__ __launch_bounds__(DB) void select_init_kernel(SelectState* st, int N, unsigned* hist)
{
    if (threadIdx.x == 0) { st->prefix = 0u; st->mask = 0u; st->rank = (unsigned)((N - 1) / 2); st->nan = 0u; }
    hist[threadIdx.x] = 0u;
}

// histogram of byte `shift` among the elements whose already-fixed bits equal the prefix
__global__ __launch_bounds__(DB) void select_hist_kernel(const float* __restrict__ gt, const float* __restrict__ rd, int N, int shift,
                                                         SelectState* __restrict__ st, unsigned* __restrict__ hist)
{
    __shared__ unsigned s_h[256];
    __shared__ unsigned s_nan;
    s_h[threadIdx.x] = 0u;
    if (threadIdx.x == 0) s_nan = 0u;
    __syncthreads();
    const unsigned prefix = st->prefix, mask = st->mask;
    for (int i = blockIdx.x * DB * 8 + threadIdx.x, it = 0; it < 8; it++, i += DB) {
        if (i >= N) break;
        const float e = hsr_depth_error(gt[i], rd[i]);
        const unsigned bits = __float_as_uint(e);
        if ((bits & mask) == prefix) atomicAdd(&s_h[(bits >> shift) & 255u], 1u);
        if (shift == 24 && e != e) atomicAdd(&s_nan, 1u);   // counted once, in the first pass; st->nan is read by the last pick only
    }
    __syncthreads();
    if (s_h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], s_h[threadIdx.x]);   // integer atomics: order-independent
    if (threadIdx.x == 0 && s_nan) atomicAdd(&st->nan, s_nan);
}

__global__ __launch_bounds__(DB) void select_pick_kernel(SelectState* st, unsigned* hist, int shift, float* out_median)
{
    __shared__ unsigned s_h[256];
    s_h[threadIdx.x] = hist[threadIdx.x];
    hist[threadIdx.x] = 0u;   // ready for the next pass
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned rank = st->rank, d = 0;
    for (; d < 255u; d++) {
        if (rank < s_h[d]) break;
        rank -= s_h[d];
    }
    unsigned prefix = st->prefix | (d << shift);
    if (shift == 0 && st->nan) prefix = 0x7fc00000u;   // the mask and emit kernels read the median from st->prefix: NaN * factor is NaN
    st->prefix = prefix;
    st->mask |= 255u << shift;
    st->rank = rank;
    if (shift == 0 && out_median) *out_median = __uint_as_float(prefix);
}

__device__ __forceinline__ bool non_presence(float sil, float rd, float gt, float sil_thres, float thr)
{
    const float derr = hsr_depth_error(gt, rd);
    const bool by_depth = (rd > gt) && (derr > thr);
    return ((sil < sil_thres) || by_depth) && (gt > 0.f);
}

__global__ __launch_bounds__(DB) void mask_count_kernel(const float* __restrict__ sil, const float* __restrict__ rd,
                                                        const float* __restrict__ gt, int N, float sil_thres, float depth_factor,
                                                        const SelectState* __restrict__ st, unsigned* __restrict__ counts,
                                                        uint8_t* __restrict__ out_mask)
{
    __shared__ unsigned s_w[4];
    const int i = blockIdx.x * DB + threadIdx.x;
    const float thr = depth_factor * __uint_as_float(st->prefix);   // 50 * depth_error.median()
    const bool m = i < N && non_presence(sil[i], rd[i], gt[i], sil_thres, thr);
    if (out_mask && i < N) out_mask[i] = m ? 1 : 0;
    const unsigned n = hsr_block256_count(m, s_w);
    if (threadIdx.x == 0) counts[blockIdx.x] = n;
}

__global__ __launch_bounds__(1024) void scan_counts_kernel(int nblk, unsigned* __restrict__ counts, int* __restrict__ out_count)
{
    __shared__ unsigned s_w[17];
    const unsigned total = hsr_block1024_exclusive_scan(nblk, counts, s_w);
    if (threadIdx.x == 0) *out_count = (int)total;
}

__global__ __launch_bounds__(DB) void emit_points_kernel(const float* __restrict__ sil, const float* __restrict__ rd,
                                                         const float* __restrict__ gt, const float* __restrict__ color, int W, int N,
                                                         hsr_pinhole f, const float* __restrict__ c2w, float sil_thres, float depth_factor,
                                                         const SelectState* __restrict__ st, const unsigned* __restrict__ offsets,
                                                         int capacity, float* __restrict__ out_means, float* __restrict__ out_rgb,
                                                         float* __restrict__ out_log_scales, float* __restrict__ out_msd)
{
    __shared__ unsigned s_w[4];
    const int i = blockIdx.x * DB + threadIdx.x;
    const float thr = depth_factor * __uint_as_float(st->prefix);
    const float z = i < N ? gt[i] : 0.f;
    const bool m = i < N && non_presence(sil[i], rd[i], z, sil_thres, thr);
    const unsigned rank = hsr_block_rank<4>(m, s_w);   // holds the barrier: no thread returns before it
    if (!m) return;
    const unsigned pos = offsets[blockIdx.x] + rank;
    if (pos >= (unsigned)capacity) return;
    const int py = i / W, px = i - py * W;
    hsr_backproject((float)px, (float)py, z, f, c2w, out_means + 3 * pos);
#pragma unroll
    for (int c = 0; c < 3; c++) out_rgb[3 * pos + c] = color[(size_t)c * N + i];
    const float sg = hsr_depth_scale(z, f);
    const float msd = sg * sg;
    if (out_msd) out_msd[pos] = msd;
    out_log_scales[pos] = logf(sqrtf(msd));        // :1157
}

// ---- prune + concat of the map (utils/slam_external.py:121-188) as ONE order-preserving row compaction --------------------
// keep mask of prune_gaussians (:175-180): to_remove = sigmoid(logit_opacity) < threshold  |  max_c exp(log_scale_c) > big
__global__ __launch_bounds__(DB) void prune_mask_kernel(int P, int S, const float* __restrict__ logit, const float* __restrict__ lscale,
                                                        float thr, float big, uint8_t* __restrict__ keep, unsigned* __restrict__ counts)
{
    __shared__ unsigned s_w[4];
    const int i = blockIdx.x * DB + threadIdx.x;
    bool k = false;
    if (i < P) {
        const float sg = 1.0f / (1.0f + expf(-logit[i]));          // torch.sigmoid
        bool rem = sg < thr;
        if (big > 0.f && lscale) {
            float m = expf(lscale[(size_t)i * S]);
            for (int c = 1; c < S; c++) {   // torch's max(dim=1): a NaN column makes the maximum NaN (fmaxf would drop it)
                const float v = expf(lscale[(size_t)i * S + c]);
                m = (v > m || v != v) ? v : m;
            }
            rem = rem || (m > big);         // NaN > big is false: such a row is not removed for its size
        }
        k = !rem;
        keep[i] = k ? 1 : 0;
    }
    const unsigned n = hsr_block256_count(k, s_w);
    if (threadIdx.x == 0) counts[blockIdx.x] = n;
}
__global__ __launch_bounds__(DB) void count_keep_kernel(int P, const uint8_t* __restrict__ keep, unsigned* __restrict__ counts)
{
    __shared__ unsigned s_w[4];
    const int i = blockIdx.x * DB + threadIdx.x;
    const unsigned n = hsr_block256_count(i < P && keep[i] != 0, s_w);
    if (threadIdx.x == 0) counts[blockIdx.x] = n;
}
__global__ void add_int_kernel(int* v, int base, int add, int overwrite) { *v = (overwrite ? base : *v) + add; }
struct RowTables {
    int n;
    hsr_row_table t[HSR_MAX_ROW_TABLES];
};
// rows [0, P): kept rows move to their rank (block offset + ballot rank: source order is preserved, which is what
// `tensor[to_keep]` yields); rows [P, P + n_append): the appended rows (or zeros: fresh Adam moments) land behind them
__global__ __launch_bounds__(DB) void compact_append_kernel(int P, int n_append, const uint8_t* __restrict__ keep,
                                                            const unsigned* __restrict__ offsets, const int* __restrict__ kept_total,
                                                            RowTables tb)
{
    __shared__ unsigned s_w[4];
    const int i = blockIdx.x * DB + threadIdx.x;
    const int nblk_keep = (P + DB - 1) / DB;
    if ((int)blockIdx.x < nblk_keep) {
        const bool k = i < P && (!keep || keep[i] != 0);
        const unsigned rank = hsr_block_rank<4>(k, s_w);   // holds the barrier: no thread of these blocks returns before it
        if (!k) return;
        const size_t pos = (size_t)(keep ? offsets[blockIdx.x] : (unsigned)(blockIdx.x * DB)) + rank;
        for (int t = 0; t < tb.n; t++) {
            const int C = tb.t[t].cols;
            const float* src = tb.t[t].src + (size_t)i * C;
            float* dst = tb.t[t].dst + pos * C;
            for (int c = 0; c < C; c++) dst[c] = src[c];
        }
        return;
    }
    const int a = i - nblk_keep * DB;
    if (a >= n_append) return;
    const size_t pos = (size_t)(keep ? *kept_total : P) + a;
    for (int t = 0; t < tb.n; t++) {
        const int C = tb.t[t].cols;
        float* dst = tb.t[t].dst + pos * C;
        const float* app = tb.t[t].append;
        for (int c = 0; c < C; c++) dst[c] = app ? app[(size_t)a * C + c] : 0.f;
    }
}

}  // namespace

extern "C" size_t hsr_compact_scratch_bytes(int P)
{
    const size_t nblk = ((size_t)(P > 0 ? P : 1) + DB - 1) / DB;
    return hsr_align256(nblk * sizeof(unsigned)) + 512;
}

extern "C" int hsr_prune_mask(int P, int S, const float* logit_opacities, const float* log_scales, float removal_opacity_threshold,
                              float big_world_threshold, uint8_t* out_keep, int* out_kept, char* scratch, size_t scratch_bytes,
                              void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || !out_kept || (P > 0 && (!logit_opacities || !out_keep)) || (big_world_threshold > 0.f && (S < 1 || !log_scales))) {
        hsr_set_error("prune_mask: invalid arguments (P=%d S=%d)", P, S);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (int rc = hsr_check_scratch("prune_mask", scratch, scratch_bytes, hsr_compact_scratch_bytes(P))) return rc;
    unsigned* counts = reinterpret_cast<unsigned*>(scratch);
    const int nblk = (P + DB - 1) / DB;
    if (P > 0)
        prune_mask_kernel<<<nblk, DB, 0, stream>>>(P, S, logit_opacities, log_scales, removal_opacity_threshold, big_world_threshold,
                                                   out_keep, counts);
    scan_counts_kernel<<<1, 1024, 0, stream>>>(nblk, counts, out_kept);   // counts -> exclusive offsets (what compact needs), total
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_compact_append_rows(int P, const uint8_t* keep, int keep_is_scanned, int n_tables, const hsr_row_table* tables,
                                       int n_append, int* out_rows, char* scratch, size_t scratch_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || n_append < 0 || n_tables < 0 || n_tables > HSR_MAX_ROW_TABLES || (n_tables > 0 && !tables) || !out_rows) {
        hsr_set_error("compact_append_rows: invalid arguments (P=%d n_append=%d n_tables=%d, at most %d tables)", P, n_append, n_tables,
                      HSR_MAX_ROW_TABLES);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    RowTables tb;
    tb.n = n_tables;
    for (int t = 0; t < n_tables; t++) {
        tb.t[t] = tables[t];
        if (tb.t[t].cols < 1 || !tb.t[t].dst || (P > 0 && !tb.t[t].src)) {
            hsr_set_error("compact_append_rows: table %d needs cols >= 1, dst and (for P > 0) src", t);
            return HSR_ERR_INVALID_ARGUMENT;
        }
    }
    if (int rc = hsr_check_scratch("compact_append_rows", scratch, scratch_bytes, hsr_compact_scratch_bytes(P))) return rc;
    unsigned* counts = reinterpret_cast<unsigned*>(scratch);
    const int nblk = (P + DB - 1) / DB;
    if (keep && !keep_is_scanned) {   // a caller-made mask: count and scan it here
        if (P > 0) count_keep_kernel<<<nblk, DB, 0, stream>>>(P, keep, counts);
        scan_counts_kernel<<<1, 1024, 0, stream>>>(nblk, counts, out_rows);
    }
    const int ablk = (n_append + DB - 1) / DB;
    if (nblk + ablk > 0 && n_tables > 0)
        compact_append_kernel<<<nblk + ablk, DB, 0, stream>>>(P, n_append, keep, counts, out_rows, tb);
    add_int_kernel<<<1, 1, 0, stream>>>(out_rows, keep ? 0 : P, n_append, keep ? 0 : 1);   // out_rows = kept + appended
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" size_t hsr_densify_scratch_bytes(int H, int W)
{
    if (H < 1 || W < 1) return 4096;
    const size_t nblk = ((size_t)H * W + DB - 1) / DB;
    return 256 + hsr_align256(256 * sizeof(unsigned)) + hsr_align256(nblk * sizeof(unsigned)) + 1024;
}

extern "C" int hsr_densify_frame(int H, int W, const float* silhouette, const float* render_depth, const float* gt_depth,
                                 const float* color, float fx, float fy, float cx, float cy, const float* c2w, float sil_thres,
                                 float depth_factor, int capacity, int* out_count, float* out_means3D, float* out_rgb,
                                 float* out_log_scales, float* out_mean_sq_dist, uint8_t* out_mask, float* out_median, char* scratch,
                                 size_t scratch_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (hsr_bad_frame_size(H, W) || !silhouette || !render_depth || !gt_depth || !color || !c2w || !out_count) {
        hsr_set_error("densify_frame: invalid sizes H=%d W=%d or NULL silhouette/render_depth/gt_depth/color/c2w/out_count", H, W);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (capacity < 0 || (capacity > 0 && (!out_means3D || !out_rgb || !out_log_scales))) {
        hsr_set_error("densify_frame: capacity=%d needs out_means3D, out_rgb and out_log_scales", capacity);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (int rc = hsr_check_scratch("densify_frame", scratch, scratch_bytes, hsr_densify_scratch_bytes(H, W))) return rc;
    const int N = H * W;
    const int nblk = (N + DB - 1) / DB;
    SelectState* st = reinterpret_cast<SelectState*>(scratch);
    unsigned* hist = reinterpret_cast<unsigned*>(scratch + 256);
    unsigned* counts = reinterpret_cast<unsigned*>(scratch + 256 + hsr_align256(256 * sizeof(unsigned)));
    select_init_kernel<<<1, DB, 0, stream>>>(st, N, hist);
    const int hblk = (N + DB * 8 - 1) / (DB * 8);
    for (int shift = 24; shift >= 0; shift -= 8) {
        select_hist_kernel<<<hblk, DB, 0, stream>>>(gt_depth, render_depth, N, shift, st, hist);
        select_pick_kernel<<<1, DB, 0, stream>>>(st, hist, shift, out_median);
    }
    mask_count_kernel<<<nblk, DB, 0, stream>>>(silhouette, render_depth, gt_depth, N, sil_thres, depth_factor, st, counts, out_mask);
    scan_counts_kernel<<<1, 1024, 0, stream>>>(nblk, counts, out_count);
    if (capacity > 0) {
        hsr_pinhole f{fx, fy, cx, cy};
        emit_points_kernel<<<nblk, DB, 0, stream>>>(silhouette, render_depth, gt_depth, color, W, N, f, c2w, sil_thres, depth_factor, st,
                                                    counts, capacity, out_means3D, out_rgb, out_log_scales, out_mean_sq_dist);
    }
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}
