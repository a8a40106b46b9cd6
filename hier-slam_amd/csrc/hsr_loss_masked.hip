// hsr_loss_masked.hip — the masked-L1 loss head (gfx950), DESIGN.md §7: the depth and colour terms of the reference's get_loss*
// (scripts/hierslam.py:903-937) behind two ABIs that differ in one factor of the mask:
//   hsr_loss_tracking_* (include/hsr_losses.h):          mask = (gt > 0) & ~isnan(d) [& (silhouette > sil_thres)]
//   hsr_loss_outlier_*  (include/ext/hsr_loss_outlier.h): the same & (|gt - d| * (gt > 0) < 10 * median of that error over the map),
//                                                         the ignore_outlier_depth_loss branch (:909-913)
// What it replaces: six mask kernels, two boolean gathers, two abs / sum chains and their autograd, and with rejection a dozen more (sub,
// abs, gt, mul, median = a sort of H*W values, mul, lt, and, ...) and a bool mask tensor.  Here the mask lives in a register.
//   value_kernel<OUTLIER>  : both masked sums and the selection count of a workgroup's pixels; one partial per workgroup.  The OUTLIER
//                            instance first finds the three digits of the median again (24 KB of reads) and forms the threshold.
//   finish_kernel          : fixed-order sum of the partials in double; terms, weighted total, 1 / selected pixels.
//   grad_kernel            : when autograd asks; the mask recomputed (with rejection: from the threshold in device memory).
// The exact median is a radix select over the bits of the error, which is never negative and therefore orders as an unsigned integer:
// 11 + 11 + 10 bits in three launches.
//   hist_kernel<0|1|2> : every workgroup counts the digit of its pixels (pass 1 and 2: of those that agree with the digits already
//                        decided) into a 2048-bin histogram in LDS and adds its non-zero bins into the pass's global histogram with
//                        integer atomics.  Passes 1 and 2 begin with EVERY workgroup finding the bin that holds the rank in the
//                        global histograms of the launches before (8 KB each, finished: the kernel boundary is the only
//                        synchronisation; no workgroup reads within a launch what another wrote in it).  A NaN counter rides along.
// Integer counts throughout the selection, fixed-order float sums: every output is the same bits on every run.
// Compiled with -ffp-contract=off: error and threshold are computed as written.  Denormals are kept (hipcc's default for fp32 on gfx9).
#include "hsr_common.h"
#include "hsr_block.h"
#include "../../include/ext/hsr_loss_outlier.h"

namespace {

constexpr int LB = 256;               // threads per workgroup
constexpr int ITEMS = 4;              // pixels per thread: the grid is ceil(N / (LB * ITEMS)) until a cap stops it
constexpr int MAX_BLOCKS = 512;       // with rejection; then the workgroups stride: 2 per CU; each pays a 2048-bin clear, flush and up to three rank searches
constexpr int BINS = 2048;            // 11 bits; the last pass uses 1024 of them
constexpr int HIST_WORDS = 3 * BINS;  // the three global histograms, then the control words
constexpr int CTL_NAN = HIST_WORDS;   // number of NaN errors
constexpr size_t ZERO_BYTES = (size_t)(HIST_WORDS + 4) * sizeof(unsigned);      // 24592: a multiple of 16, from the scratch's start
constexpr size_t PART_OFF = hsr_align256(ZERO_BYTES);                           // float partials [MAX_BLOCKS][2]
constexpr size_t COUNT_OFF = PART_OFF + (size_t)MAX_BLOCKS * 2 * sizeof(float); // unsigned selected [MAX_BLOCKS]
constexpr size_t SCRATCH_BYTES = COUNT_OFF + (size_t)MAX_BLOCKS * sizeof(unsigned);

// the mask of a pixel; reject: additionally the error below the threshold (strict: a NaN threshold selects nothing).  Not thr = +inf for
// the plain mask: an infinite depth on a valid pixel has the error inf, inf < inf is false, and the plain mask selects that pixel
__device__ __forceinline__ bool selected(bool reject, float gt, float d, float thr, float sil, float sil_thres, int use_sil)
{
    return (!reject || hsr_depth_error(gt, d) < thr) && gt > 0.f && !(d != d) && (!use_sil || sil > sil_thres);
}

struct Rank { unsigned bin, rank; };

// The bin of hist[0 .. LB * PER) that holds the element of 0-based rank `rank`, and the rank of that element inside the bin.  All LB
// threads call it; `hist` was finished by an earlier launch.  A rank beyond the total (it never is: every pixel is counted) gives {0, 0}.
template <int PER>
__device__ __forceinline__ Rank find_bin(const unsigned* hist, unsigned rank, unsigned* s_wave, unsigned* s_res)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned c[PER], t = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) {
        c[k] = hist[threadIdx.x * PER + k];
        t += c[k];
    }
    unsigned incl = hsr_wave_inclusive_scan(t, lane);
    if (threadIdx.x == 0) s_res[0] = s_res[1] = 0;
    if (lane == 63) s_wave[wv] = incl;
    __syncthreads();
    for (int w = 0; w < wv; w++) incl += s_wave[w];
    const unsigned excl = incl - t;
    if (excl <= rank && rank < incl) {      // exactly one thread
        unsigned r = rank - excl, bin = PER - 1;
        bool found = false;
#pragma unroll
        for (int k = 0; k < PER; k++)
            if (!found) {
                if (r < c[k]) {
                    bin = k;
                    found = true;
                } else {
                    r -= c[k];
                }
            }
        s_res[0] = threadIdx.x * PER + bin;
        s_res[1] = r;
    }
    __syncthreads();
    const Rank out{s_res[0], s_res[1]};
    __syncthreads();      // s_wave / s_res are free for the next search
    return out;
}

// PASS 0: bits 31..21 of every error;  1: bits 20..10 of those whose bits 31..21 hold the rank;  2: bits 9..0 of those whose bits 31..10 do
template <int PASS>
__global__ __launch_bounds__(LB) void hist_kernel(const float* __restrict__ depth, const float* __restrict__ gt_depth, unsigned N,
                                                  unsigned* hist /* [HIST_WORDS + 4] */)
{
    __shared__ unsigned s_hist[BINS];
    __shared__ unsigned s_wave[LB / 64], s_res[2];
    for (int b = threadIdx.x; b < BINS; b += LB) s_hist[b] = 0;
    unsigned prefix = 0;
    if (PASS >= 1) {
        const Rank a = find_bin<BINS / LB>(hist, (N - 1) / 2, s_wave, s_res);
        prefix = a.bin;
        if (PASS == 2) prefix = (a.bin << 11) | find_bin<BINS / LB>(hist + BINS, a.rank, s_wave, s_res).bin;
    }
    __syncthreads();
    unsigned nan = 0;
    for (unsigned i = blockIdx.x * LB + threadIdx.x; i < N; i += gridDim.x * LB) {      // i + stride < 2^31 + 2^17
        const float e = hsr_depth_error(gt_depth[i], depth[i]);
        const unsigned key = __float_as_uint(e);      // key >> 21 <= 2047 whatever the bits
        if (PASS == 0) {
            nan += e != e ? 1u : 0u;
            atomicAdd(&s_hist[key >> 21], 1u);
        } else if (PASS == 1) {
            if ((key >> 21) == prefix) atomicAdd(&s_hist[(key >> 10) & 0x7ffu], 1u);
        } else {
            if ((key >> 10) == prefix) atomicAdd(&s_hist[key & 0x3ffu], 1u);
        }
    }
    __syncthreads();
    unsigned* out = hist + PASS * BINS;
    for (int b = threadIdx.x; b < (PASS == 2 ? 1024 : BINS); b += LB) {
        const unsigned c = s_hist[b];
        if (c) atomicAdd(&out[b], c);
    }
    if (PASS == 0) {
        nan = hsr_wave_sum(nan);
        if ((threadIdx.x & 63) == 0 && nan) atomicAdd(&hist[CTL_NAN], nan);
    }
}

// the median from the three finished histograms; all LB threads
__device__ __forceinline__ float block_median(const unsigned* hist, unsigned N, unsigned* s_wave, unsigned* s_res)
{
    const Rank a = find_bin<BINS / LB>(hist, (N - 1) / 2, s_wave, s_res);
    const Rank b = find_bin<BINS / LB>(hist + BINS, a.rank, s_wave, s_res);
    const Rank c = find_bin<1024 / LB>(hist + 2 * BINS, b.rank, s_wave, s_res);
    const unsigned key = (a.bin << 21) | (b.bin << 10) | c.bin;
    return hist[CTL_NAN] ? __uint_as_float(0x7fc00000u) : __uint_as_float(key);
}

__global__ __launch_bounds__(LB) void median_kernel(const unsigned* hist, unsigned N, float* __restrict__ out2)
{
    __shared__ unsigned s_wave[LB / 64], s_res[2];
    const float med = block_median(hist, N, s_wave, s_res);
    if (threadIdx.x == 0) {
        out2[0] = med;
        out2[1] = 10.0f * med;
    }
}

// OUTLIER: the threshold from the finished histograms, one pixel per thread and trip (the grid is capped at MAX_BLOCKS and strides);
// otherwise no threshold, ITEMS pixels per thread and a grid that covers N in one trip.  Either way a thread adds its terms in index order.
template <bool OUTLIER>
__global__ __launch_bounds__(LB) void value_kernel(const float* __restrict__ im, const float* __restrict__ gt_im, int C,
                                                   const float* __restrict__ depth, const float* __restrict__ gt_depth,
                                                   const float* __restrict__ sil, float sil_thres, int use_sil, unsigned N,
                                                   const unsigned* hist, float* __restrict__ partials /* [nblk][2]: depth sum, colour sum */,
                                                   unsigned* __restrict__ counts /* [nblk]: selected pixels */, float* __restrict__ out6)
{
    constexpr unsigned PER = OUTLIER ? 1 : ITEMS;
    __shared__ unsigned s_wave[LB / 64], s_res[2];
    __shared__ float s_red[LB / 64];
    float thr = 0.f;
    if constexpr (OUTLIER) {
        const float med = block_median(hist, N, s_wave, s_res);
        thr = 10.0f * med;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            out6[4] = med;
            out6[5] = thr;
        }
    }
    float acc_d = 0.f, acc_c = 0.f;
    unsigned n = 0;
    for (unsigned base = blockIdx.x * LB * PER; base < N; base += gridDim.x * LB * PER)      // no wrap: base < N < 2^31, stride < N + LB * PER
#pragma unroll
        for (unsigned it = 0; it < PER; it++) {
            const unsigned i = base + threadIdx.x + it * LB;
            if (i >= N) break;
            const float gd = gt_depth[i], d = depth[i];
            const bool sel = selected(OUTLIER, gd, d, thr, use_sil ? sil[i] : 1.f, sil_thres, use_sil);
            acc_d += sel ? fabsf(gd - d) : 0.f;
            n += sel ? 1u : 0u;
            for (int c = 0; c < C; c++) {
                const float e = fabsf(gt_im[(size_t)c * N + i] - im[(size_t)c * N + i]);
                acc_c += sel ? e : 0.f;
            }
        }
    const float td = hsr_block256_sum(acc_d, s_red);
    const float tc = hsr_block256_sum(acc_c, s_red);
    const unsigned tn = hsr_block256_isum(n, s_wave);   // s_wave is idle: find_bin ends with a barrier
    if (threadIdx.x == 0) {
        partials[2 * (size_t)blockIdx.x] = td;
        partials[2 * (size_t)blockIdx.x + 1] = tc;
        counts[blockIdx.x] = tn;
    }
}

// out[0] = depth term, out[1] = colour term, out[2] = w_depth * out[0] + w_im * out[1], out[3] = 1 / selected pixels; *out_selected if asked.
// mean: the terms are means over the selection (colour: tiled over its C planes); an empty selection gives NaN like torch.
// Thread t sums partials t, t + 256, ... in double, then a halving tree: a fixed order.
__global__ __launch_bounds__(LB) void finish_kernel(const float* __restrict__ partials, const unsigned* __restrict__ counts, int nblocks,
                                                    float w_depth, float w_im, int mean, int C, float* __restrict__ out,
                                                    int* __restrict__ out_selected /* may be NULL */)
{
    __shared__ double s_acc[LB][2];
    __shared__ unsigned s_cnt[LB];
    double a0 = 0.0, a1 = 0.0;
    unsigned n = 0;      // < 2^31
    for (int b = threadIdx.x; b < nblocks; b += LB) {
        a0 += (double)partials[2 * (size_t)b];
        a1 += (double)partials[2 * (size_t)b + 1];
        n += counts[b];
    }
    s_acc[threadIdx.x][0] = a0;
    s_acc[threadIdx.x][1] = a1;
    s_cnt[threadIdx.x] = n;
    __syncthreads();
    for (int o = LB / 2; o >= 1; o >>= 1) {
        if (threadIdx.x < o) {
            s_acc[threadIdx.x][0] += s_acc[threadIdx.x + o][0];
            s_acc[threadIdx.x][1] += s_acc[threadIdx.x + o][1];
            s_cnt[threadIdx.x] += s_cnt[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float inv = 1.0f / (float)s_cnt[0];
        const double dterm = mean ? s_acc[0][0] * (double)inv : s_acc[0][0];
        const double cterm = mean ? (C > 0 ? s_acc[0][1] * (double)inv / (double)C : 0.0) : s_acc[0][1];
        out[0] = (float)dterm;
        out[1] = (float)cterm;
        // One fused multiply-add, written out so that the file's -ffp-contract=off does not decide it: the tracking entry has always
        // rounded here once (its finish was compiled with contraction: v_mul_f64, v_fmac_f64).  The outlier entry used to round the
        // depth product as well; its out6[2] can differ from that only where the double lies within one double-ulp of an fp32 rounding
        // boundary, and then by one fp32 ulp.
        out[2] = (float)fma((double)w_depth, dterm, (double)w_im * cterm);
        out[3] = inv;
        if (out_selected) out_selected[0] = (int)s_cnt[0];
    }
}

// threshold == NULL: the plain mask.  Up to 65536 workgroups, then they stride: i + stride < 2^31 + 2^24
__global__ __launch_bounds__(LB) void grad_kernel(const float* __restrict__ im, const float* __restrict__ gt_im, int C,
                                                  const float* __restrict__ depth, const float* __restrict__ gt_depth,
                                                  const float* __restrict__ sil, float sil_thres, int use_sil, unsigned N,
                                                  const float* __restrict__ threshold, const float* __restrict__ upstream, float w_depth,
                                                  float w_im, const float* __restrict__ inv_count, float* __restrict__ d_im,
                                                  float* __restrict__ d_depth)
{
    const bool reject = threshold != nullptr;
    const float thr = reject ? threshold[0] : 0.f;
    const float up = upstream ? upstream[0] : 1.0f;
    const float inv = inv_count ? inv_count[0] : 1.0f;   // mean reduction: 1 / selected pixels (the value pass's out[3])
    const float sd = w_depth * up * inv, sc = w_im * up * (inv_count ? inv / (float)(C > 0 ? C : 1) : 1.0f);
    for (unsigned i = blockIdx.x * LB + threadIdx.x; i < N; i += gridDim.x * LB) {
        const float gd = gt_depth[i], d = depth[i];
        const bool sel = selected(reject, gd, d, thr, use_sil ? sil[i] : 1.f, sil_thres, use_sil);
        if (d_depth) {
            const float e = d - gd;   // d |gt - d| / d d = sign(d - gt)
            d_depth[i] = sel ? (e > 0.f ? sd : (e < 0.f ? -sd : 0.f)) : 0.f;
        }
        if (d_im)
            for (int c = 0; c < C; c++) {
                const float e = im[(size_t)c * N + i] - gt_im[(size_t)c * N + i];
                d_im[(size_t)c * N + i] = sel ? (e > 0.f ? sc : (e < 0.f ? -sc : 0.f)) : 0.f;
            }
    }
}

// ceil(N / (LB * ITEMS)) workgroups, at least one, at most `cap`
unsigned blocks_for(unsigned N, unsigned cap)
{
    const unsigned nb = (N + LB * ITEMS - 1) / (LB * ITEMS);
    return nb < 1 ? 1 : (nb > cap ? cap : nb);
}

// the tracking entry's scratch: float [nb][2], then unsigned [nb], nb uncapped
size_t tracking_bytes(int H, int W)
{
    const size_t nb = ((size_t)H * W + LB * ITEMS - 1) / (LB * ITEMS);
    return hsr_align256(nb * 3 * sizeof(float));
}

// any_c: the tracking ABI takes every C >= 0, the outlier ABI 0 or 3
int check_maps(const char* who, bool any_c, int C, int H, int W, const float* im, const float* gt_im, const float* depth,
               const float* gt_depth, const float* sil, int use_sil)
{
    if (hsr_bad_frame_size(H, W) || !depth || !gt_depth) {
        hsr_set_error("%s: invalid sizes H=%d W=%d (H, W >= 1, H * W < 2^31) or NULL depth / gt_depth", who, H, W);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (C < 0 || (!any_c && C != 0 && C != 3) || (C > 0 && (!im || !gt_im)) || (use_sil && !sil)) {
        hsr_set_error("%s: C=%d is %s, or NULL im / gt_im / silhouette", who, C, any_c ? "negative" : "neither 0 nor 3");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    return HSR_OK;
}

// zeroing + the three histogram passes; leaves the finished histograms at the scratch's start
int launch_select(unsigned N, int nb, const float* depth, const float* gt_depth, char* scratch, hipStream_t stream)
{
    unsigned* hist = reinterpret_cast<unsigned*>(scratch);
    HSR_HIP_CHECK(hipMemsetAsync(scratch, 0, ZERO_BYTES, stream));
    hist_kernel<0><<<nb, LB, 0, stream>>>(depth, gt_depth, N, hist);
    hist_kernel<1><<<nb, LB, 0, stream>>>(depth, gt_depth, N, hist);
    hist_kernel<2><<<nb, LB, 0, stream>>>(depth, gt_depth, N, hist);
    return HSR_OK;
}

// both value entries.  reject: the outlier one (out = out6, out_selected required, its fixed scratch layout)
int masked_value(const char* who, bool reject, int C, int H, int W, const float* im, const float* gt_im, const float* depth,
                 const float* gt_depth, const float* sil, float sil_thres, int use_sil, int reduction, float w_depth, float w_im, float* out,
                 int* out_selected, char* scratch, size_t scratch_bytes, hipStream_t stream)
{
    int rc = check_maps(who, !reject, C, H, W, im, gt_im, depth, gt_depth, sil, use_sil);
    if (rc != HSR_OK) return rc;
    if (!out || (reject && !out_selected) || (reduction != HSR_LOSS_SUM && reduction != HSR_LOSS_MEAN)) {
        hsr_set_error("%s: out%s is NULL or reduction is neither HSR_LOSS_SUM nor HSR_LOSS_MEAN", who, reject ? "6 / out_selected" : "4");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    rc = reject ? hsr_check_scratch(who, scratch, scratch_bytes, SCRATCH_BYTES, 16) : hsr_check_scratch(who, scratch, scratch_bytes, tracking_bytes(H, W), 4);
    if (rc != HSR_OK) return rc;
    const unsigned N = (unsigned)H * (unsigned)W;
    const int nb = (int)blocks_for(N, reject ? MAX_BLOCKS : ~0u);
    float* partials = reinterpret_cast<float*>(reject ? scratch + PART_OFF : scratch);
    unsigned* counts = reject ? reinterpret_cast<unsigned*>(scratch + COUNT_OFF) : reinterpret_cast<unsigned*>(partials + 2 * (size_t)nb);
    if (reject) {
        rc = launch_select(N, nb, depth, gt_depth, scratch, stream);
        if (rc != HSR_OK) return rc;
        value_kernel<true><<<nb, LB, 0, stream>>>(im, gt_im, C, depth, gt_depth, sil, sil_thres, use_sil, N,
                                                  reinterpret_cast<const unsigned*>(scratch), partials, counts, out);
    } else {
        value_kernel<false><<<nb, LB, 0, stream>>>(im, gt_im, C, depth, gt_depth, sil, sil_thres, use_sil, N, nullptr, partials, counts, out);
    }
    finish_kernel<<<1, LB, 0, stream>>>(partials, counts, nb, w_depth, w_im, reduction == HSR_LOSS_MEAN ? 1 : 0, C, out, out_selected);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

// both gradient entries.  threshold == NULL: the tracking one
int masked_grad(const char* who, int C, int H, int W, const float* im, const float* gt_im, const float* depth, const float* gt_depth,
                const float* sil, float sil_thres, int use_sil, float w_depth, float w_im, const float* threshold, const float* upstream,
                const float* inv_count, float* d_im, float* d_depth, hipStream_t stream)
{
    const int rc = check_maps(who, !threshold, C, H, W, im, gt_im, depth, gt_depth, sil, use_sil);
    if (rc != HSR_OK) return rc;
    const unsigned N = (unsigned)H * (unsigned)W;
    if (C == 0) d_im = nullptr;
    if (!d_im && !d_depth) return HSR_OK;      // nothing asked for, nothing launched
    grad_kernel<<<blocks_for(N, 65536u), LB, 0, stream>>>(im, gt_im, C, depth, gt_depth, sil, sil_thres, use_sil, N, threshold, upstream, w_depth,
                                                          w_im, inv_count, d_im, d_depth);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

}  // namespace

extern "C" size_t hsr_loss_tracking_scratch_bytes(int H, int W)
{
    return H < 1 || W < 1 ? 1024 : tracking_bytes(H, W) + 256;
}

extern "C" int hsr_loss_tracking_value(int C, int H, int W, const float* im, const float* gt_im, const float* depth, const float* gt_depth,
                                       const float* silhouette, float sil_thres, int use_sil, int reduction, float w_depth, float w_im,
                                       float* out4, char* scratch, size_t scratch_bytes, void* stream)
{
    return masked_value("loss_tracking_value", false, C, H, W, im, gt_im, depth, gt_depth, silhouette, sil_thres, use_sil, reduction, w_depth,
                        w_im, out4, nullptr, scratch, scratch_bytes, (hipStream_t)stream);
}

extern "C" int hsr_loss_tracking_grad(int C, int H, int W, const float* im, const float* gt_im, const float* depth, const float* gt_depth,
                                      const float* silhouette, float sil_thres, int use_sil, float w_depth, float w_im, const float* upstream,
                                      const float* inv_count, float* d_im, float* d_depth, void* stream)
{
    return masked_grad("loss_tracking_grad", C, H, W, im, gt_im, depth, gt_depth, silhouette, sil_thres, use_sil, w_depth, w_im, nullptr,
                       upstream, inv_count, d_im, d_depth, (hipStream_t)stream);
}

extern "C" size_t hsr_loss_outlier_scratch_bytes(int H, int W)
{
    (void)H;
    (void)W;
    return SCRATCH_BYTES;
}

extern "C" int hsr_loss_outlier_median(int H, int W, const float* depth, const float* gt_depth, float* out2, char* scratch,
                                       size_t scratch_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    int rc = check_maps("loss_outlier_median", false, 0, H, W, nullptr, nullptr, depth, gt_depth, nullptr, 0);
    if (rc != HSR_OK) return rc;
    if (!out2) {
        hsr_set_error("loss_outlier_median: out2 is NULL");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    rc = hsr_check_scratch("loss_outlier_median", scratch, scratch_bytes, SCRATCH_BYTES, 16);
    if (rc != HSR_OK) return rc;
    const unsigned N = (unsigned)H * (unsigned)W;
    rc = launch_select(N, (int)blocks_for(N, MAX_BLOCKS), depth, gt_depth, scratch, stream);
    if (rc != HSR_OK) return rc;
    median_kernel<<<1, LB, 0, stream>>>(reinterpret_cast<const unsigned*>(scratch), N, out2);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_loss_outlier_value(int C, int H, int W, const float* im, const float* gt_im, const float* depth, const float* gt_depth,
                                      const float* silhouette, float sil_thres, int use_sil, int reduction, float w_depth, float w_im,
                                      float* out6, int* out_selected, char* scratch, size_t scratch_bytes, void* stream)
{
    return masked_value("loss_outlier_value", true, C, H, W, im, gt_im, depth, gt_depth, silhouette, sil_thres, use_sil, reduction, w_depth,
                        w_im, out6, out_selected, scratch, scratch_bytes, (hipStream_t)stream);
}

extern "C" int hsr_loss_outlier_grad(int C, int H, int W, const float* im, const float* gt_im, const float* depth, const float* gt_depth,
                                     const float* silhouette, float sil_thres, int use_sil, float w_depth, float w_im, const float* threshold,
                                     const float* upstream, const float* inv_count, float* d_im, float* d_depth, void* stream)
{
    if (!threshold) {
        hsr_set_error("loss_outlier_grad: threshold is NULL (pass &out6[5] of the value pass)");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    return masked_grad("loss_outlier_grad", C, H, W, im, gt_im, depth, gt_depth, silhouette, sil_thres, use_sil, w_depth, w_im, threshold,
                       upstream, inv_count, d_im, d_depth, (hipStream_t)stream);
}
