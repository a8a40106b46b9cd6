// hsr_losses.hip — fused loss heads on the rendered maps (gfx950), SURVEY.md §8(f) rank 2.
//
// What it replaces in the reference: the torch eager chains of get_loss_semantic_mlp (scripts/hierslam.py:921-1016) —
// boolean-mask gathers + abs + sum/mean for depth and colour, calc_ssim's five grouped conv2d calls and their autograd
// (utils/slam_external.py:66-97), and per tree level a permute + view + CrossEntropyLoss (log_softmax, nll_loss and
// their backward) over a channel slice of the K logit planes (scripts/hierslam.py:91-111, :963-974).
// Here every head is ONE streaming pass over the planar maps that yields the value and the gradient together:
//   * L1: value = block partial sums -> fixed-order finish; gradient = sign * scale written in the same pass (the
//     selection count of a masked mean comes from a byte-wide pre-pass over the mask);
//   * SSIM: 32x32-pixel tiles with a 5-pixel halo of both images in LDS, the reference's Gaussian applied as two
//     11-tap passes with sliding register windows; the forward pass also writes the three partial-derivative maps, the
//     backward pass is the adjoint correlation of those;
//   * tree cross-entropy: one thread per pixel walks the levels, channels are read with stride H*W (coalesced across
//     the wave); a level of up to 16 channels sits in registers (exact max, then sum), a wider one is streamed with an
//     online log-sum-exp; the value pass counts the valid labels, the gradient pass writes softmax - onehot straight
//     into the planar gradient — no [H*W, n] permute.
// All HBM-bound; algorithmic bytes per pixel: L1 4C*3 (+1 mask), SSIM 4C*(2 + 3) fwd + 4C*(3 + 2 + 1) bwd, CE 4K*3 + 8L.
// The tracking loss of include/hsr_losses.h (hsr_loss_tracking_*: mask, both masked sums and their gradients as one head) is not here: it
// shares its kernels with the outlier-rejecting head in hsr_loss_masked.hip.
#include "hsr_common.h"
#include "hsr_block.h"
#include "hsr_tree.h"
#include "../../include/hsr_losses.h"
#include <cmath>

namespace {

constexpr int LB = 256;          // threads per block of the streaming kernels
constexpr int L1_ITEMS = 8;      // pixels per thread (L1)
constexpr int SS_T = 32;         // SSIM tile edge (256 threads x 2x2 outputs)
constexpr int SS_R = 5;          // window radius (11x11)
constexpr int SS_E = SS_T + 2 * SS_R;

// ---------------------------------------------------------------- finish: fixed-order sum of per-block partials
// out[k] = scale_k * sum_b partials[b * stride + k];  scale: 1, or *inv (device), see `mode`
__global__ __launch_bounds__(LB) void finish_kernel(const float* __restrict__ partials, int nblocks, int stride, int nout,
                                                    const float* __restrict__ inv, float host_scale, float* __restrict__ out)
{
    __shared__ double s_acc[LB];
    for (int k = 0; k < nout; k++) {
        double acc = 0.0;
        for (int b = threadIdx.x; b < nblocks; b += LB) acc += (double)partials[(size_t)b * stride + k];
        s_acc[threadIdx.x] = acc;
        __syncthreads();
        for (int o = LB / 2; o > 0; o >>= 1) {
            if (threadIdx.x < o) s_acc[threadIdx.x] += s_acc[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            double v = s_acc[0] * (double)host_scale;
            if (inv) v *= (double)inv[k];
            out[k] = (float)v;
        }
        __syncthreads();
    }
}

// counts -> reciprocal:  inv[k] = 1 / sum_b partials[b*stride + k]   (NaN-free: 0 count gives +inf, which makes the mean
// NaN exactly like torch's mean over an empty selection and the gradient 0 * inf = NaN only where selected — nowhere)
__global__ __launch_bounds__(LB) void count_finish_kernel(const unsigned* __restrict__ partials, int nblocks, int stride, int nout,
                                                          float* __restrict__ inv)
{
    __shared__ unsigned long long s_acc[LB];
    for (int k = 0; k < nout; k++) {
        unsigned long long acc = 0;
        for (int b = threadIdx.x; b < nblocks; b += LB) acc += partials[(size_t)b * stride + k];
        s_acc[threadIdx.x] = acc;
        __syncthreads();
        for (int o = LB / 2; o > 0; o >>= 1) {
            if (threadIdx.x < o) s_acc[threadIdx.x] += s_acc[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) inv[k] = 1.0f / (float)s_acc[0];
        __syncthreads();
    }
}

// ---------------------------------------------------------------- L1
__global__ __launch_bounds__(LB) void mask_count_kernel(const uint8_t* __restrict__ mask, int N, unsigned* __restrict__ partials)
{
    __shared__ unsigned s_red[4];
    unsigned c = 0;
    for (int i = blockIdx.x * LB * L1_ITEMS + threadIdx.x, it = 0; it < L1_ITEMS; it++, i += LB)
        if (i < N) c += mask[i] != 0;
    const unsigned total = hsr_block256_isum(c, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// grid: (blocks over N, C).  scale = host_scale * (inv ? inv[0] : 1)
__global__ __launch_bounds__(LB) void l1_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                const uint8_t* __restrict__ mask, int N, const float* __restrict__ inv,
                                                float host_scale, float* __restrict__ grad, float* __restrict__ partials)
{
    __shared__ float s_red[4];
    const size_t plane = (size_t)blockIdx.y * N;
    const float scale = host_scale * (inv ? inv[0] : 1.0f);
    float acc = 0.f;
    for (int i = blockIdx.x * LB * L1_ITEMS + threadIdx.x, it = 0; it < L1_ITEMS; it++, i += LB) {
        if (i >= N) break;
        const bool sel = mask ? mask[i] != 0 : true;
        const float d = pred[plane + i] - gt[plane + i];
        // unselected pixels contribute nothing, whatever they hold (the reference's mask exists to exclude NaN depths)
        acc += sel ? fabsf(d) : 0.f;
        if (grad) grad[plane + i] = sel ? (d > 0.f ? scale : (d < 0.f ? -scale : 0.f)) : 0.f;
    }
    const float tot = hsr_block256_sum(acc, s_red);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

// ---------------------------------------------------------------- SSIM
// The reference's window is the outer product of a normalised 11-tap Gaussian with itself (utils/slam_external.py:60-62),
// so the 121-tap correlation is evaluated as a horizontal then a vertical 11-tap pass (the two differ from the 2-D form by
// one fp32 rounding per weight).  Tile = 32x32 outputs, 42x42 inputs in LDS; both passes slide a 14-value register window
// over 4 consecutive outputs, so a pixel costs ~27 LDS reads and ~130 FMAs instead of 242 and 605.
template <int NQ>
__device__ __forceinline__ void blur4(const float (&v)[NQ][14], const hsr_gauss& gw, float (&out)[NQ][4])
{
#pragma unroll
    for (int q = 0; q < NQ; q++)
#pragma unroll
        for (int o = 0; o < 4; o++) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 11; k++) acc = fmaf(gw.g[k], v[q][o + k], acc);
            out[q][o] = acc;
        }
}

// grid (tiles_x, tiles_y, C); block 256
__global__ __launch_bounds__(LB) void ssim_forward_kernel(const float* __restrict__ img1, const float* __restrict__ img2, int H, int W,
                                                          hsr_gauss gw, float* __restrict__ d_mu1, float* __restrict__ d_s11,
                                                          float* __restrict__ d_s12, float* __restrict__ partials)
{
    __shared__ float s_x[SS_E][SS_E + 1], s_y[SS_E][SS_E + 1];
    __shared__ float s_h[5][SS_E][SS_T + 1];   // horizontally blurred x, y, xx, yy, xy
    __shared__ float s_red[4];
    const size_t plane = (size_t)blockIdx.z * H * W;
    const int x0 = blockIdx.x * SS_T - SS_R, y0 = blockIdx.y * SS_T - SS_R;
    for (int i = threadIdx.x; i < SS_E * SS_E; i += LB) {
        const int ly = i / SS_E, lx = i - ly * SS_E;
        const int gx = x0 + lx, gy = y0 + ly;
        const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;   // zero padding (conv2d padding = 5)
        const size_t o = plane + (size_t)(in ? gy : 0) * W + (in ? gx : 0);
        const float a = img1[o], b = img2[o];
        s_x[ly][lx] = in ? a : 0.f;
        s_y[ly][lx] = in ? b : 0.f;
    }
    __syncthreads();
    // pass 1: rows 0..41, 8 groups of 4 columns each
    for (int item = threadIdx.x; item < SS_E * (SS_T / 4); item += LB) {
        const int r = item / (SS_T / 4), c0 = (item % (SS_T / 4)) * 4;
        float v[5][14];
#pragma unroll
        for (int k = 0; k < 14; k++) {
            const float a = s_x[r][c0 + k], b = s_y[r][c0 + k];
            v[0][k] = a; v[1][k] = b; v[2][k] = a * a; v[3][k] = b * b; v[4][k] = a * b;
        }
        float o4[5][4];
        blur4<5>(v, gw, o4);
#pragma unroll
        for (int q = 0; q < 5; q++)
#pragma unroll
            for (int o = 0; o < 4; o++) s_h[q][r][c0 + o] = o4[q][o];
    }
    __syncthreads();
    // pass 2: thread = (column, group of 4 rows)
    const int col = threadIdx.x & 31, r0 = (threadIdx.x >> 5) * 4;
    float v[5][14];
#pragma unroll
    for (int q = 0; q < 5; q++)
#pragma unroll
        for (int k = 0; k < 14; k++) v[q][k] = s_h[q][r0 + k][col];
    float m[5][4];
    blur4<5>(v, gw, m);
    const float c1 = 0.01f * 0.01f, c2 = 0.03f * 0.03f;
    float acc = 0.f;
    const int px = blockIdx.x * SS_T + col;
#pragma unroll
    for (int o = 0; o < 4; o++) {
        const int py = blockIdx.y * SS_T + r0 + o;
        const float m1 = m[0][o], m2 = m[1][o];
        const float mu1_sq = m1 * m1, mu2_sq = m2 * m2, mu12 = m1 * m2;
        const float sig1 = m[2][o] - mu1_sq, sig2 = m[3][o] - mu2_sq, sig12 = m[4][o] - mu12;
        const float A1 = 2.f * mu12 + c1, A2 = 2.f * sig12 + c2, B1 = mu1_sq + mu2_sq + c1, B2 = sig1 + sig2 + c2;
        const float inv12 = 1.0f / (B1 * B2);
        const float smap = (A1 * A2) * inv12;
        const bool live = px < W && py < H;
        if (live && d_mu1) {
            const size_t off = plane + (size_t)py * W + px;
            d_mu1[off] = (2.f * m2 * A2 - 2.f * m2 * A1) * inv12 - smap * (2.f * m1 / B1 - 2.f * m1 / B2);
            d_s11[off] = -smap / B2;
            d_s12[off] = 2.f * A1 * inv12;
        }
        acc += live ? smap : 0.f;
    }
    const float tot = hsr_block256_sum(acc, s_red);
    if (threadIdx.x == 0) partials[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = tot;
}

// adjoint of the zero-padded correlation with a symmetric window = the same correlation of the three partial-derivative
// maps (which are zero outside the image)
__global__ __launch_bounds__(LB) void ssim_backward_kernel(const float* __restrict__ img1, const float* __restrict__ img2, int H, int W,
                                                           hsr_gauss gw, const float* __restrict__ d_mu1, const float* __restrict__ d_s11,
                                                           const float* __restrict__ d_s12, float inv_n_host, const float* __restrict__ upstream,
                                                           float* __restrict__ grad)
{
    const float inv_n = inv_n_host * (upstream ? upstream[0] : 1.0f);   // the node's incoming gradient, read on the device (hsr_loss_ssim_grad)
    __shared__ float s_in[3][SS_E][SS_E + 1];
    __shared__ float s_h[3][SS_E][SS_T + 1];
    const size_t plane = (size_t)blockIdx.z * H * W;
    const int x0 = blockIdx.x * SS_T - SS_R, y0 = blockIdx.y * SS_T - SS_R;
    for (int i = threadIdx.x; i < SS_E * SS_E; i += LB) {
        const int ly = i / SS_E, lx = i - ly * SS_E;
        const int gx = x0 + lx, gy = y0 + ly;
        const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
        const size_t o = plane + (size_t)(in ? gy : 0) * W + (in ? gx : 0);
        const float m = d_mu1[o], a = d_s11[o], b = d_s12[o];
        s_in[0][ly][lx] = in ? m : 0.f;
        s_in[1][ly][lx] = in ? a : 0.f;
        s_in[2][ly][lx] = in ? b : 0.f;
    }
    __syncthreads();
    for (int item = threadIdx.x; item < SS_E * (SS_T / 4); item += LB) {
        const int r = item / (SS_T / 4), c0 = (item % (SS_T / 4)) * 4;
        float v[3][14];
#pragma unroll
        for (int q = 0; q < 3; q++)
#pragma unroll
            for (int k = 0; k < 14; k++) v[q][k] = s_in[q][r][c0 + k];
        float o4[3][4];
        blur4<3>(v, gw, o4);
#pragma unroll
        for (int q = 0; q < 3; q++)
#pragma unroll
            for (int o = 0; o < 4; o++) s_h[q][r][c0 + o] = o4[q][o];
    }
    __syncthreads();
    const int col = threadIdx.x & 31, r0 = (threadIdx.x >> 5) * 4;
    float v[3][14];
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
        for (int k = 0; k < 14; k++) v[q][k] = s_h[q][r0 + k][col];
    float gsum[3][4];
    blur4<3>(v, gw, gsum);
    const int px = blockIdx.x * SS_T + col;
#pragma unroll
    for (int o = 0; o < 4; o++) {
        const int py = blockIdx.y * SS_T + r0 + o;
        if (px < W && py < H) {
            const size_t off = plane + (size_t)py * W + px;
            grad[off] = (gsum[0][o] + 2.f * img1[off] * gsum[1][o] + img2[off] * gsum[2][o]) * inv_n;
        }
    }
}

// ---------------------------------------------------------------- tree cross-entropy
struct Levels : hsr_tree_levels {
    float weight[HSR_LOSS_MAX_LEVELS];
};

// valid labels (!= ignore_index) of ONE label plane per block: the leaf head's count (the tree kernel counts in its value pass)
__global__ __launch_bounds__(LB) void valid_label_count_kernel(const int64_t* __restrict__ labels, int N, int ignore_index,
                                                               unsigned* __restrict__ partials)
{
    __shared__ unsigned s_red[4];
    const int i = blockIdx.x * LB + threadIdx.x;
    const unsigned total = hsr_block256_count(i < N && labels[i] != (int64_t)ignore_index, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// Two passes: the value pass counts the valid labels itself and writes no gradient; the gradient pass runs when autograd asks for it
// and multiplies by the upstream gradient it reads from device memory — no label pre-pass, no stashed K x H x W gradient, no
// `stash * g` multiply afterwards (at 1200 x 680, K = 26: 76 + 35 + 23 us of launches became 2 passes of 118 and 203 MB).
// A level of at most CE_REG channels is held in registers: all its loads go out together, one expf per channel, no second read.
constexpr int CE_REG = 16;

constexpr int CE_ITEMS = 1;   // pixels per thread (2 was measured: 41 + 47 us against 37 + 41 — fewer independent loads in flight per lane than two threads give)

// TB: threads per block — the value pass runs 1 024 (a quarter of the block partials for its one-block finisher), the gradient pass 256
template <bool GRAD, int TB>
__global__ __launch_bounds__(TB) void tree_ce_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, int N, int K,
                                                     Levels lv, int ignore_index, const float* __restrict__ inv_count,
                                                     const float* __restrict__ upstream, float* __restrict__ grad,
                                                     float* __restrict__ partials /* [nblk][2 * MAX_LEVELS]: loss sums, then counts */,
                                                     const float* __restrict__ add_grad, const float* __restrict__ add_scale, float add_host_scale)
{
    // GRAD: out = tree part + add_grad * (add_scale[0] * add_host_scale) — another head's stashed gradient of the same map (the leaf head's)
    // joins here instead of costing its own `stash * g` pass and autograd's add of the two K x H x W maps
    const float as = (GRAD && add_grad) ? (add_scale ? add_scale[0] : 1.0f) * add_host_scale : 0.f;
    __shared__ float s_part[TB / 64][2 * HSR_LOSS_MAX_LEVELS];   // per wave: loss sums, counts (each wave adds into its own row: no atomics)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (!GRAD && lane < 2 * HSR_LOSS_MAX_LEVELS) s_part[wv][lane] = 0.f;
    const float up = GRAD ? (upstream ? upstream[0] : 1.0f) : 0.f;
#pragma unroll 1
    for (int it = 0; it < CE_ITEMS; it++) {
        const int i = (blockIdx.x * CE_ITEMS + it) * TB + (int)threadIdx.x;
        const bool live = i < N;
        const size_t p = live ? (size_t)i : 0;
        int covered_end = 0;
#pragma unroll 1
        for (int l = 0; l < lv.n; l++) {
            const int b = lv.begin[l], n = lv.size[l];
            const int64_t lab64 = labels[(size_t)l * N + p];
            const bool valid = live && lab64 != (int64_t)ignore_index;
            const int lab = (int)lab64;
            const float sc = GRAD ? (valid ? lv.weight[l] * inv_count[l] * up : 0.f) : 0.f;
            float loss = 0.f;
            if (n <= CE_REG) {
                float z[CE_REG];
#pragma unroll
                for (int c = 0; c < CE_REG; c++) z[c] = c < n ? logits[(size_t)(b + min(c, n - 1)) * N + p] : -INFINITY;
                float m = z[0];
#pragma unroll
                for (int c = 1; c < CE_REG; c++) m = fmaxf(m, z[c]);
                float s = 0.f, picked = 0.f;
#pragma unroll
                for (int c = 0; c < CE_REG; c++) {
                    picked = (c == lab && c < n) ? z[c] : picked;   // slots c >= n hold -inf: an out-of-range label matches no class
                    z[c] = c < n ? expf(z[c] - m) : 0.f;
                    s += z[c];
                }
                if (GRAD) {
                    const float inv_s = 1.0f / s;
                    if (live) {
#pragma unroll
                        for (int c = 0; c < CE_REG; c++)
                            if (c < n) {
                                const size_t gi = (size_t)(b + c) * N + p;
                                const float tv = (z[c] * inv_s - (c == lab ? 1.f : 0.f)) * sc;
                                grad[gi] = add_grad ? fmaf(add_grad[gi], as, tv) : tv;
                            }
                    }
                } else {
                    loss = valid ? (m + logf(s)) - picked : 0.f;
                }
            } else {
                // wide level: stream it (online log-sum-exp, second read from L2)
                float m = -INFINITY, s = 0.f, picked = 0.f;
                for (int c = 0; c < n; c++) {
                    const float z = logits[(size_t)(b + c) * N + p];
                    const float nm = fmaxf(m, z);
                    s = s * expf(m - nm) + expf(z - nm);
                    m = nm;
                    picked = c == lab ? z : picked;
                }
                if (GRAD) {
                    const float inv_s = 1.0f / s;
                    if (live)
                        for (int c = 0; c < n; c++) {
                            const float z = logits[(size_t)(b + c) * N + p];
                            const size_t gi = (size_t)(b + c) * N + p;
                            const float tv = (expf(z - m) * inv_s - (c == lab ? 1.f : 0.f)) * sc;
                            grad[gi] = add_grad ? fmaf(add_grad[gi], as, tv) : tv;
                        }
                } else {
                    loss = valid ? (m + logf(s)) - picked : 0.f;
                }
            }
            if (!GRAD) {
                // the wave's sums of this level, added into the wave's own row (counts are exact in fp32: <= 64 per add, <= 128 per row)
                const float a = hsr_wave_sum(loss), cnt = hsr_wave_sum(valid ? 1.f : 0.f);
                if (lane == 0) {
                    s_part[wv][l] += a;
                    s_part[wv][HSR_LOSS_MAX_LEVELS + l] += cnt;
                }
            }
            covered_end = b + n;
        }
        if (GRAD && live)
            for (int c = covered_end; c < K; c++) grad[(size_t)c * N + p] = add_grad ? add_grad[(size_t)c * N + p] * as : 0.f;   // channels behind the last level
    }
    if (GRAD) return;
    __syncthreads();
    if (threadIdx.x < 2 * HSR_LOSS_MAX_LEVELS) {
        const int k = threadIdx.x;
        float v = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < TB / 64; w2++) v += s_part[w2][k];   // fixed order
        partials[(size_t)blockIdx.x * (2 * HSR_LOSS_MAX_LEVELS) + k] = (k % HSR_LOSS_MAX_LEVELS) < lv.n ? v : 0.f;
    }
}

// one block of 1024: level l -> loss sum / count and 1 / count, fixed order, in double.  Thread t sums column t % 32 of rows t / 32,
// t / 32 + 32, ... with four independent loads in flight (a serial walk of 3 188 rows by 8 row groups took 94 us: latency, not bytes).
constexpr int CEF_T = 1024;
__global__ __launch_bounds__(CEF_T) void tree_ce_finish_kernel(const float* __restrict__ partials, int nblocks, int num_levels,
                                                               float* __restrict__ out_level_loss, float* __restrict__ out_inv_count)
{
    constexpr int COLS = 2 * HSR_LOSS_MAX_LEVELS, ROWS = CEF_T / COLS;
    __shared__ double s_acc[ROWS][COLS + 1];
    __shared__ double s_tot[COLS];
    const int k = threadIdx.x % COLS, j = threadIdx.x / COLS;
    double acc = 0.0;
    if ((k % HSR_LOSS_MAX_LEVELS) < num_levels) {
        int b = j;
        for (; b + 3 * ROWS < nblocks; b += 4 * ROWS) {
            const float v0 = partials[(size_t)b * COLS + k], v1 = partials[(size_t)(b + ROWS) * COLS + k];
            const float v2 = partials[(size_t)(b + 2 * ROWS) * COLS + k], v3 = partials[(size_t)(b + 3 * ROWS) * COLS + k];
            acc += ((double)v0 + (double)v1) + ((double)v2 + (double)v3);
        }
        for (; b < nblocks; b += ROWS) acc += (double)partials[(size_t)b * COLS + k];
    }
    s_acc[j][k] = acc;
    __syncthreads();
    if (threadIdx.x < COLS) {
        double v = 0.0;
        for (int r = 0; r < ROWS; r++) v += s_acc[r][threadIdx.x];
        s_tot[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x < num_levels) {
        // 0 valid labels: 1 / 0 = +inf and 0 * inf = NaN, torch's mean over an empty selection; the gradient pass writes 0 there
        const float inv = 1.0f / (float)s_tot[HSR_LOSS_MAX_LEVELS + threadIdx.x];
        out_inv_count[threadIdx.x] = inv;
        out_level_loss[threadIdx.x] = (float)(s_tot[threadIdx.x] * (double)inv);
    }
}

// ---------------------------------------------------------------- leaf head: 1x1-conv MLP + cross-entropy, fused
// logits[c] = b[c] + sum_k Wt[c][k] * sem[k]  per pixel (torch.nn.Conv2d(K, C, 1), scripts/hierslam.py:1756), CrossEntropyLoss on
// them (scripts/hierslam.py:976-983), and the three gradients.  One thread per pixel (lane = pixel):
//   pass 1: the C logits on the fly -> online log-sum-exp;  weights are wave-uniform, i.e. scalar loads + v_fmac with an SGPR;
//   pass 2, 16 classes at a time: logits again, g = (softmax - onehot) / count, d_sem[k] += Wt[c][k] * g  (VALU), and g goes
//           into a per-wave LDS panel [16 classes][64 pixels];  d_Wt[c][k] = sum_pixels g[c] * sem[k] is a GEMM with the
//           reduction over pixels, so it runs on the matrix cores: A = the panel (class, pixel), B = sem of the wave's 64
//           pixels transposed once through LDS into B-operand layout, v_mfma_f32_16x16x4_f32 (exact fp32 fmaf chain), the
//           C x K accumulators stay in registers over all pixels a workgroup visits.  The bias is input channel K (constant
//           1), so d_b is column K of d_Wt.
// Neither the [C,H,W] logits nor their gradient ever exist in memory (333 MB each at C = 102, 1200x680).
// Workgroups are persistent (grid = a few per CU) so that the per-workgroup partial d_Wt fits a fixed-order finish.
constexpr int LM_MAX_BLOCKS = 768;   // persistent workgroups (3 per CU)
constexpr int LM_KP = 32;           // padded input width: K channels + bias input, K <= 31
constexpr int LM_MAX_CT = 8;        // class tiles of 16: C <= 128
constexpr int LM_PANEL = 64 * 17;   // floats per wave: max(16 * 66, 64 * 17)
constexpr int LM_STRIDE = 66;
typedef float lm_f32x4 __attribute__((ext_vector_type(4)));
typedef float lm_f32x2 __attribute__((ext_vector_type(2)));

// KU: input columns actually multiplied (K channels + the bias input, rounded up to 4); CT: class tiles in use (<= 8)
template <int KU, int MAXCT>
__global__ void __launch_bounds__(256, 3) leaf_mlp_ce_kernel(const float* __restrict__ sem, const float* __restrict__ wt /*[C][LM_KP], bias at K*/,
                                                             const int64_t* __restrict__ labels, int N, int K, int C, int CT, int ignore_index,
                                                             const float* __restrict__ inv_count, float* __restrict__ d_sem,
                                                             float* __restrict__ part_loss, float* __restrict__ part_dw)
{
    __shared__ float s_panel[4][LM_PANEL];
    __shared__ float s_st[4][LM_KP][65];   // sem of the wave's 64 pixels, [channel][pixel]: B operand of the weight-gradient GEMM
    __shared__ float s_red[4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    float* panel = s_panel[wv];
    lm_f32x4 acc[MAXCT][2];
#pragma unroll
    for (int ct = 0; ct < MAXCT; ct++)
#pragma unroll
        for (int nt = 0; nt < 2; nt++) acc[ct][nt] = lm_f32x4{0.f, 0.f, 0.f, 0.f};
    float loss_acc = 0.f;
    const float inv = inv_count[0];

    for (int base = blockIdx.x * 256; base < N; base += gridDim.x * 256) {
        const int px = base + t;
        const bool live = px < N;
        const size_t p = live ? (size_t)px : 0;
        float sv[LM_KP];
#pragma unroll
        for (int k = 0; k < LM_KP; k++) sv[k] = k < K ? sem[(size_t)k * N + p] : 0.f;   // unconditional loads, then masked
#pragma unroll
        for (int k = 0; k < LM_KP; k++) sv[k] = k < K ? (live ? sv[k] : 0.f) : (k == K && live ? 1.0f : 0.f);
        const int64_t lab64 = labels[p];
        const bool valid = live && lab64 != (int64_t)ignore_index;
        const int lab = (int)lab64;

        // B operand of the weight-gradient GEMM: sem of this wave's 64 pixels, parked in LDS as [channel][pixel] (kept in
        // registers it would cost 32 of them and the third wave per SIMD)
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < LM_KP; k++) s_st[wv][k][lane] = sv[k];
        __builtin_amdgcn_wave_barrier();
        // The weight row of the NEXT class is fetched (scalar loads: the address is wave-uniform) while the current class is
        // evaluated; exponentials are v_exp_f32 on pre-scaled arguments (2 instructions instead of libm's 14 — the logits
        // are O(10), so the extra rounding of z*log2(e) is ~1e-6 relative, inside the 1e-5 the tests ask for).
        auto load_row = [&](int c, float (&w)[KU]) {
            const float4* w4 = reinterpret_cast<const float4*>(wt + (size_t)min(c, CT * 16 - 1) * LM_KP);
#pragma unroll
            for (int q = 0; q < KU / 4; q++) {
                const float4 x = w4[q];
                w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w;
            }
        };
        constexpr float L2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

        // pass 1: log-sum-exp of the C logits, in base 2 (m2 = running max of z*log2e, sum of 2^(z*log2e - m2))
        float m2 = -INFINITY, sum = 0.f, picked = 0.f;
        {
            auto class1 = [&](int c, const float (&w)[KU]) {
                // no contraction here: z2 - nm must use the ROUNDED z2 that the running maximum and `picked` hold.  Contracted to
                // fma(z, log2e, -nm) it leaves the rounding residual of z2 in the exponent, 2^residual is 1 or 1 + 2^-23, and a one-class
                // head's log-sum-exp is no longer its logit: the loss is then ~1e-7 per pixel, not 0
#pragma clang fp contract(off)
                // two interleaved partial sums: the pairs (w[2j], w[2j+1]) x (sv[2j], sv[2j+1]) become v_pk_fma_f32 — half the
                // instructions of a 28-deep v_fmac chain, and the kernel's time is the instructions it issues
                lm_f32x2 zz = {0.f, 0.f};
#pragma unroll
                for (int k = 0; k < KU; k += 2) zz = __builtin_elementwise_fma(lm_f32x2{w[k], w[k + 1]}, lm_f32x2{sv[k], sv[k + 1]}, zz);
                const float z = zz.x + zz.y;
                const float z2 = z * L2E;
                picked = c == lab ? z2 : picked;   // in base 2, like the log-sum-exp it is subtracted from
                const float nm = fmaxf(m2, z2);
                sum = fmaf(sum, __builtin_amdgcn_exp2f(m2 - nm), __builtin_amdgcn_exp2f(z2 - nm));
                m2 = nm;
            };
            // two register sets, ping-pong (rotating one set into the other costs a scalar move per weight per class, and a
            // wave issues one instruction per 4 cycles whatever its type)
            float wa[KU], wb[KU];
            load_row(0, wa);
            for (int c = 0; c < C; c += 2) {
                load_row(c + 1, wb);
                class1(c, wa);
                load_row(c + 2, wa);
                if (c + 1 < C) class1(c + 1, wb);
            }
        }
        // log2-sum-exp2;  lse = lse2 * ln 2.  The label's logit is subtracted before that scaling: both terms carry the same rounding of
        // z * log2(e), so a one-class head loses exactly 0 (lse2 * ln 2 - z does not: the two roundings leave ~1e-7 |z| per pixel)
        const float lse2 = m2 + __builtin_amdgcn_logf(sum);
        loss_acc += valid ? (lse2 - picked) * LN2 : 0.f;
        const float gscale = valid ? inv : 0.f;

        // pass 2: gradients.  A runtime loop over the classes (the class arithmetic exists once in the code: unrolling it
        // per 16-class tile made hipcc keep several tiles' weights in flight and spill ~900 SGPRs); every 16th class
        // the panel goes through the matrix cores into that tile's accumulators.
        float ds[LM_KP];
#pragma unroll
        for (int k = 0; k < LM_KP; k++) ds[k] = 0.f;
        {
            auto class2 = [&](int c, const float (&w)[KU]) {
                lm_f32x2 zz = {0.f, 0.f};   // as in pass 1 (the same summation order: the softmax of pass 2 is that of pass 1's log-sum-exp)
#pragma unroll
                for (int k = 0; k < KU; k += 2) zz = __builtin_elementwise_fma(lm_f32x2{w[k], w[k + 1]}, lm_f32x2{sv[k], sv[k + 1]}, zz);
                const float z = zz.x + zz.y;
                // rows >= C of the packed weights are zero: z = 0 there, and the class must not contribute
                const float g = c < C ? (__builtin_amdgcn_exp2f(fmaf(z, L2E, -lse2)) - (c == lab ? 1.f : 0.f)) * gscale : 0.f;
#pragma unroll
                for (int k = 0; k < KU; k++) ds[k] = fmaf(w[k], g, ds[k]);
                panel[(c & 15) * LM_STRIDE + lane] = g;
                if ((c & 15) == 15) {
                    __builtin_amdgcn_wave_barrier();
                    const float* arow = panel + (lane & 15) * LM_STRIDE + (lane >> 4);
                    float av[16];
#pragma unroll
                    for (int m = 0; m < 16; m++) av[m] = arow[4 * m];
                    // B[k = pixel 4m + (lane>>4)][n = channel 16nt + (lane&15)]
                    const float* brow = &s_st[wv][lane & 15][lane >> 4];
#pragma unroll
                    for (int ct = 0; ct < MAXCT; ct++)
                        if (ct == (c >> 4)) {   // wave-uniform: static accumulator index
#pragma unroll
                            for (int m = 0; m < 16; m++) {
                                acc[ct][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], brow[4 * m], acc[ct][0], 0, 0, 0);
                                acc[ct][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], brow[16 * 65 + 4 * m], acc[ct][1], 0, 0, 0);
                            }
                        }
                    __builtin_amdgcn_wave_barrier();
                }
            };
            float wa[KU], wb[KU];
            load_row(0, wa);
            for (int c = 0; c < CT * 16; c += 2) {
                load_row(c + 1, wb);
                class2(c, wa);
                load_row(c + 2, wa);
                class2(c + 1, wb);
            }
        }
        if (live && d_sem)
#pragma unroll
            for (int k = 0; k < LM_KP; k++)
                if (k < K) d_sem[(size_t)k * N + p] = ds[k];
    }

    // ---- per-workgroup partials: loss, then d_Wt[c][k] summed over the four waves in a fixed order ----
    const float tot = hsr_block256_sum(loss_acc, s_red);
    if (t == 0) part_loss[blockIdx.x] = tot;
    float* out = part_dw + (size_t)blockIdx.x * (CT * 16 * LM_KP);
#pragma unroll
    for (int ct = 0; ct < MAXCT; ct++)
#pragma unroll
        for (int nt = 0; nt < 2; nt++) {
            if (ct >= CT) break;   // uniform
            // D[row = 4*(lane>>4) + r][col = lane&15]: class 16ct + row, input channel 16nt + col
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 4; r++) panel[(4 * (lane >> 4) + r) * 17 + (lane & 15)] = acc[ct][nt][r];
            __syncthreads();
            {
                const int row = t >> 4, col = t & 15;   // 256 threads = 16 x 16 outputs
                const float v = ((s_panel[0][row * 17 + col] + s_panel[1][row * 17 + col]) + s_panel[2][row * 17 + col]) +
                                s_panel[3][row * 17 + col];
                out[(size_t)(16 * ct + row) * LM_KP + 16 * nt + col] = v;
            }
        }
}

// weights [C][K] + bias [C] -> rows of LM_KP floats: Wt[c][k<K] = weight, Wt[c][K] = bias, 0 elsewhere (rows >= C zero)
__global__ __launch_bounds__(256) void leaf_pack_weights_kernel(const float* __restrict__ weight, const float* __restrict__ bias, int K, int C,
                                                                int rows, float* __restrict__ wt)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * LM_KP) return;
    const int c = i / LM_KP, k = i - c * LM_KP;
    wt[i] = c < C ? (k < K ? weight[(size_t)c * K + k] : (k == K ? bias[c] : 0.f)) : 0.f;
}

// d_weight[c][k], d_bias[c] = fixed-order sum over the workgroup partials (double): 32 outputs x 8 partial-groups per
// workgroup, groups combined through LDS in index order
// (32 partial-groups of a 1 024-thread block, four loads in flight per thread: with 8 groups walking 96 partials each, one after the
// other, the launch took 30 us for 11 MB)
constexpr int LFD_T = 1024, LFD_G = LFD_T / 32;
__global__ __launch_bounds__(LFD_T) void leaf_finish_dw_kernel(const float* __restrict__ part_dw, int nblk, int per, int K, int C,
                                                               float* __restrict__ d_weight, float* __restrict__ d_bias)
{
    __shared__ double s_acc[LFD_G][33];
    const int o = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + o;
    double acc = 0.0;
    if (i < per) {
        int b = grp;
        for (; b + 3 * LFD_G < nblk; b += 4 * LFD_G) {
            const float v0 = part_dw[(size_t)b * per + i], v1 = part_dw[(size_t)(b + LFD_G) * per + i];
            const float v2 = part_dw[(size_t)(b + 2 * LFD_G) * per + i], v3 = part_dw[(size_t)(b + 3 * LFD_G) * per + i];
            acc += ((double)v0 + (double)v1) + ((double)v2 + (double)v3);
        }
        for (; b < nblk; b += LFD_G) acc += (double)part_dw[(size_t)b * per + i];
    }
    s_acc[grp][o] = acc;
    __syncthreads();
    if (grp != 0 || i >= per) return;
    double tot = 0.0;
#pragma unroll
    for (int g2 = 0; g2 < LFD_G; g2++) tot += s_acc[g2][o];
    const int c = i / LM_KP, k = i - c * LM_KP;
    if (c >= C || k > K) return;
    if (k < K) { if (d_weight) d_weight[(size_t)c * K + k] = (float)tot; }
    else if (d_bias) d_bias[c] = (float)tot;
}

}  // namespace

extern "C" size_t hsr_loss_scratch_bytes(int channels, int H, int W)
{
    if (channels < 1 || H < 1 || W < 1) return 1024;
    const size_t N = (size_t)H * W;
    const size_t tiles = (size_t)((W + SS_T - 1) / SS_T) * ((H + SS_T - 1) / SS_T);
    const size_t blocks = (N + LB - 1) / LB + 1;
    // SSIM: three partial-derivative maps + one partial per tile;  L1: small;  CE: the term is kept as callers' allocations know it
    // (MAX_LEVELS partials per 256-pixel block, twice).  hsr_loss_tree_ce needs hsr_loss_tree_ce_scratch_bytes(H, W) = align256(2 x) + 256
    // with x = (blocks - 1) * MAX_LEVELS floats, and align256(2 x) <= 2 align256(x): the term is ample
    size_t need = hsr_align256(3 * (size_t)channels * N * sizeof(float)) + hsr_align256((size_t)channels * tiles * sizeof(float));
    const size_t ce = 2 * hsr_align256(blocks * HSR_LOSS_MAX_LEVELS * sizeof(float)) + 256;
    const size_t l1 = 2 * hsr_align256((size_t)channels * blocks * sizeof(float)) + 256;
    if (ce > need) need = ce;
    if (l1 > need) need = l1;
    const size_t leaf = (size_t)LM_MAX_BLOCKS * (LM_MAX_CT * 16 * LM_KP + 4) * sizeof(float) + 2 * hsr_align256(blocks * sizeof(float)) +
                        (size_t)LM_MAX_CT * 16 * LM_KP * sizeof(float) + 4096;
    if (leaf > need) need = leaf;
    return need + 1024;
}

extern "C" int hsr_loss_l1(int C, int H, int W, const float* pred, const float* gt, const uint8_t* mask, int reduction, float* out_loss,
                           float* out_grad, char* scratch, size_t scratch_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (C < 1 || hsr_bad_frame_size(H, W) || !pred || !gt || !out_loss) {
        hsr_set_error("loss_l1: invalid sizes C=%d H=%d W=%d or NULL pred/gt/out_loss", C, H, W);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (reduction != HSR_LOSS_SUM && reduction != HSR_LOSS_MEAN) {
        hsr_set_error("loss_l1: reduction must be HSR_LOSS_SUM or HSR_LOSS_MEAN");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const int N = H * W;
    const int nb = (N + LB * L1_ITEMS - 1) / (LB * L1_ITEMS);
    const size_t part_bytes = hsr_align256((size_t)C * nb * sizeof(float));
    int rc = hsr_check_scratch("loss_l1", scratch, scratch_bytes, 2 * part_bytes + 256);
    if (rc != HSR_OK) return rc;
    float* partials = reinterpret_cast<float*>(scratch);
    unsigned* cparts = reinterpret_cast<unsigned*>(scratch + part_bytes);
    float* inv = reinterpret_cast<float*>(scratch + 2 * part_bytes);
    const float* inv_arg = nullptr;
    float host_scale = 1.0f;
    if (reduction == HSR_LOSS_MEAN) {
        if (mask) {
            mask_count_kernel<<<nb, LB, 0, stream>>>(mask, N, cparts);
            count_finish_kernel<<<1, LB, 0, stream>>>(cparts, nb, 1, 1, inv);
            inv_arg = inv;
            host_scale = 1.0f / (float)C;   // the selection is tiled over the C planes
        } else {
            host_scale = (float)(1.0 / ((double)C * N));
        }
    }
    l1_kernel<<<dim3(nb, C), LB, 0, stream>>>(pred, gt, mask, N, inv_arg, host_scale, out_grad, partials);
    finish_kernel<<<1, LB, 0, stream>>>(partials, C * nb, 1, 1, inv_arg, host_scale, out_loss);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

namespace {
dim3 ssim_grid(int C, int H, int W) { return dim3((W + SS_T - 1) / SS_T, (H + SS_T - 1) / SS_T, C); }

float ssim_inv_n(int C, int H, int W) { return (float)(1.0 / ((double)C * (double)((size_t)H * W))); }

// the mean SSIM into out_ssim; maps (3 * C * H * W floats or NULL) receives the three partial-derivative maps; partials: one float per tile
void launch_ssim_value(int C, int H, int W, const float* img1, const float* img2, float* maps, float* partials, float* out_ssim, hipStream_t stream)
{
    const size_t CN = (size_t)C * H * W;
    const dim3 grid = ssim_grid(C, H, W);
    ssim_forward_kernel<<<grid, LB, 0, stream>>>(img1, img2, H, W, hsr_gauss_window(), maps, maps ? maps + CN : nullptr, maps ? maps + 2 * CN : nullptr,
                                                 partials);
    finish_kernel<<<1, LB, 0, stream>>>(partials, (int)(grid.x * grid.y * grid.z), 1, 1, nullptr, ssim_inv_n(C, H, W), out_ssim);
}

// the adjoint correlation of the value pass's maps, times upstream[0] (DEVICE, NULL = 1)
void launch_ssim_grad(int C, int H, int W, const float* img1, const float* img2, const float* maps, const float* upstream, float* out_grad,
                      hipStream_t stream)
{
    const size_t CN = (size_t)C * H * W;
    ssim_backward_kernel<<<ssim_grid(C, H, W), LB, 0, stream>>>(img1, img2, H, W, hsr_gauss_window(), maps, maps + CN, maps + 2 * CN, ssim_inv_n(C, H, W),
                                                                upstream, out_grad);
}
}  // namespace

// One call: value and, if out_grad is given, gradient; the maps sit at the front of the scratch, then the partials.
extern "C" int hsr_loss_ssim(int C, int H, int W, const float* img1, const float* img2, float* out_ssim, float* out_grad, char* scratch,
                             size_t scratch_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (C < 1 || H < 1 || W < 1 || !img1 || !img2 || !out_ssim) {
        hsr_set_error("loss_ssim: invalid sizes C=%d H=%d W=%d or NULL img1/img2/out_ssim", C, H, W);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const dim3 grid = ssim_grid(C, H, W);
    const size_t map_bytes = out_grad ? hsr_align256((size_t)C * H * W * sizeof(float) * 3) : 0;
    int rc = hsr_check_scratch("loss_ssim", scratch, scratch_bytes, map_bytes + hsr_align256((size_t)grid.x * grid.y * C * sizeof(float)));
    if (rc != HSR_OK) return rc;
    float* maps = out_grad ? reinterpret_cast<float*>(scratch) : nullptr;
    launch_ssim_value(C, H, W, img1, img2, maps, reinterpret_cast<float*>(scratch + map_bytes), out_ssim, stream);
    if (out_grad) launch_ssim_grad(C, H, W, img1, img2, maps, nullptr, out_grad, stream);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

// Two-pass form for an autograd node: the value pass leaves the three partial-derivative maps in `maps` (3 * C * H * W floats, the
// caller's: they must live until the gradient pass), the gradient pass is the adjoint correlation times the upstream gradient.
extern "C" int hsr_loss_ssim_value(int C, int H, int W, const float* img1, const float* img2, float* out_ssim, float* maps, char* scratch,
                                   size_t scratch_bytes, void* stream_)
{
    if (C < 1 || H < 1 || W < 1 || !img1 || !img2 || !out_ssim) {
        hsr_set_error("loss_ssim_value: invalid sizes C=%d H=%d W=%d or NULL img1/img2/out_ssim", C, H, W);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const dim3 grid = ssim_grid(C, H, W);
    int rc = hsr_check_scratch("loss_ssim_value", scratch, scratch_bytes, hsr_align256((size_t)grid.x * grid.y * C * sizeof(float)));
    if (rc != HSR_OK) return rc;
    launch_ssim_value(C, H, W, img1, img2, maps, reinterpret_cast<float*>(scratch), out_ssim, (hipStream_t)stream_);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_loss_ssim_grad(int C, int H, int W, const float* img1, const float* img2, const float* maps, const float* upstream,
                                  float* out_grad, void* stream_)
{
    if (C < 1 || H < 1 || W < 1 || !img1 || !img2 || !maps || !out_grad) {
        hsr_set_error("loss_ssim_grad: invalid sizes C=%d H=%d W=%d or NULL img1/img2/maps/out_grad", C, H, W);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    launch_ssim_grad(C, H, W, img1, img2, maps, upstream, out_grad, (hipStream_t)stream_);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

// d loss / d pred of hsr_loss_l1 as its own pass, times the upstream gradient (DEVICE float, NULL = 1): sums with or without a mask and the
// unmasked mean — the masked mean needs the selection count of the value pass and keeps the one-pass form.
__global__ __launch_bounds__(LB) void l1_grad_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const uint8_t* __restrict__ mask,
                                                     int N, float host_scale, const float* __restrict__ upstream, float* __restrict__ grad)
{
    const size_t plane = (size_t)blockIdx.y * N;
    const float scale = host_scale * (upstream ? upstream[0] : 1.0f);
    for (int i = blockIdx.x * LB * L1_ITEMS + threadIdx.x, it = 0; it < L1_ITEMS; it++, i += LB) {
        if (i >= N) break;
        const bool sel = mask ? mask[i] != 0 : true;
        const float d = pred[plane + i] - gt[plane + i];
        grad[plane + i] = sel ? (d > 0.f ? scale : (d < 0.f ? -scale : 0.f)) : 0.f;
    }
}

extern "C" int hsr_loss_l1_grad(int C, int H, int W, const float* pred, const float* gt, const uint8_t* mask, int reduction,
                                const float* upstream, float* out_grad, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (C < 1 || hsr_bad_frame_size(H, W) || !pred || !gt || !out_grad) {
        hsr_set_error("loss_l1_grad: invalid sizes C=%d H=%d W=%d or NULL pred/gt/out_grad", C, H, W);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (reduction != HSR_LOSS_SUM && !(reduction == HSR_LOSS_MEAN && !mask)) {
        hsr_set_error("loss_l1_grad: sums (masked or not) and the unmasked mean only; the masked mean's gradient comes from hsr_loss_l1");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const int N = H * W;
    const int nb = (N + LB * L1_ITEMS - 1) / (LB * L1_ITEMS);
    const float host_scale = reduction == HSR_LOSS_MEAN ? (float)(1.0 / ((double)C * N)) : 1.0f;
    l1_grad_kernel<<<dim3(nb, C), LB, 0, stream>>>(pred, gt, mask, N, host_scale, upstream, out_grad);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

namespace {
// the checks of the three tree cross-entropy entry points, and their levels with the weights (NULL: 1)
int tree_ce_levels(const char* who, int K, int H, int W, int num_levels, const int* level_sizes, const float* level_weight, Levels* lv)
{
    if (K < 1 || hsr_bad_frame_size(H, W) || !level_sizes) {
        hsr_set_error("%s: invalid sizes K=%d H=%d W=%d or NULL level_sizes", who, K, H, W);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (num_levels < 1 || num_levels > HSR_LOSS_MAX_LEVELS) {
        hsr_set_error("%s: num_levels=%d outside [1, %d]", who, num_levels, HSR_LOSS_MAX_LEVELS);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const hsr_tree_extent e = hsr_parse_tree_levels(num_levels, level_sizes, lv);
    if (e.bad_level >= 0) {
        hsr_set_error("%s: level %d has %d classes", who, e.bad_level, level_sizes[e.bad_level]);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (e.sum > K) {
        hsr_set_error("%s: levels cover %d channels but the map has K=%d", who, (int)(e.sum > INT_MAX ? INT_MAX : e.sum), K);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    for (int l = 0; l < num_levels; l++) lv->weight[l] = level_weight ? level_weight[l] : 1.0f;
    return HSR_OK;
}
}  // namespace

extern "C" size_t hsr_loss_tree_ce_scratch_bytes(int H, int W)
{
    if (H < 1 || W < 1) return 1024;
    const size_t nb = ((size_t)H * W + LB - 1) / LB;
    return hsr_align256(nb * 2 * HSR_LOSS_MAX_LEVELS * sizeof(float)) + 256;
}

namespace {
constexpr int CE_VB = 1024;   // threads per block of the value pass

// level losses (means over the valid labels) and 1 / valid labels per level; partials: hsr_loss_tree_ce_scratch_bytes(H, W) - 256 bytes
void launch_tree_ce_value(int N, int K, const Levels& lv, const float* logits, const int64_t* labels, int ignore_index, float* partials,
                          float* out_level_loss, float* out_inv_count, hipStream_t stream)
{
    const int nb = (N + CE_VB * CE_ITEMS - 1) / (CE_VB * CE_ITEMS);
    tree_ce_kernel<false, CE_VB><<<nb, CE_VB, 0, stream>>>(logits, labels, N, K, lv, ignore_index, nullptr, nullptr, nullptr, partials, nullptr, nullptr, 0.f);
    tree_ce_finish_kernel<<<1, CEF_T, 0, stream>>>(partials, nb, lv.n, out_level_loss, out_inv_count);
}

// upstream[0] (DEVICE, NULL = 1) * d (sum_l weight_l * loss_l) / d logits + add_grad * add_scale[0] * add_host_scale (add_grad NULL: no join)
void launch_tree_ce_grad(int N, int K, const Levels& lv, const float* logits, const int64_t* labels, int ignore_index, const float* inv_count,
                         const float* upstream, const float* add_grad, const float* add_scale, float add_host_scale, float* out_grad,
                         hipStream_t stream)
{
    tree_ce_kernel<true, LB><<<(N + LB * CE_ITEMS - 1) / (LB * CE_ITEMS), LB, 0, stream>>>(logits, labels, N, K, lv, ignore_index, inv_count, upstream, out_grad, nullptr, add_grad,
                                                               add_scale, add_host_scale);
}
}  // namespace

// One call: the value pass and, if out_grad is given, the gradient pass; block partials at the front of the scratch, then 1 / count.
extern "C" int hsr_loss_tree_ce(int K, int H, int W, int num_levels, const int* level_sizes, const float* level_weight,
                                const float* logits, const int64_t* labels, int ignore_index, float* out_level_loss, float* out_grad,
                                char* scratch, size_t scratch_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    Levels lv;
    int rc = tree_ce_levels("loss_tree_ce", K, H, W, num_levels, level_sizes, level_weight, &lv);
    if (rc != HSR_OK) return rc;
    if (!logits || !labels || !out_level_loss) {
        hsr_set_error("loss_tree_ce: NULL logits / labels / out_level_loss");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    // hsr_loss_tree_ce_scratch_bytes: the value pass's partials and 256 bytes, here the 1 / count vector
    const size_t part_bytes = hsr_loss_tree_ce_scratch_bytes(H, W) - 256;
    rc = hsr_check_scratch("loss_tree_ce", scratch, scratch_bytes, part_bytes + 256);
    if (rc != HSR_OK) return rc;
    float* inv = reinterpret_cast<float*>(scratch + part_bytes);
    launch_tree_ce_value(H * W, K, lv, logits, labels, ignore_index, reinterpret_cast<float*>(scratch), out_level_loss, inv, stream);
    if (out_grad) launch_tree_ce_grad(H * W, K, lv, logits, labels, ignore_index, inv, nullptr, nullptr, nullptr, 0.f, out_grad, stream);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

// The two passes on their own, for an autograd node: the caller keeps out_inv_count until the gradient pass.
extern "C" int hsr_loss_tree_ce_value(int K, int H, int W, int num_levels, const int* level_sizes, const float* logits,
                                      const int64_t* labels, int ignore_index, float* out_level_loss, float* out_inv_count,
                                      char* scratch, size_t scratch_bytes, void* stream_)
{
    Levels lv;
    int rc = tree_ce_levels("loss_tree_ce_value", K, H, W, num_levels, level_sizes, nullptr, &lv);
    if (rc != HSR_OK) return rc;
    if (!logits || !labels || !out_level_loss || !out_inv_count) {
        hsr_set_error("loss_tree_ce_value: NULL logits / labels / out_level_loss / out_inv_count");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    rc = hsr_check_scratch("loss_tree_ce_value", scratch, scratch_bytes, hsr_loss_tree_ce_scratch_bytes(H, W) - 256);
    if (rc != HSR_OK) return rc;
    launch_tree_ce_value(H * W, K, lv, logits, labels, ignore_index, reinterpret_cast<float*>(scratch), out_level_loss, out_inv_count,
                         (hipStream_t)stream_);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_loss_tree_ce_grad(int K, int H, int W, int num_levels, const int* level_sizes, const float* level_weight,
                                     const float* logits, const int64_t* labels, int ignore_index, const float* inv_count,
                                     const float* upstream, const float* add_grad, const float* add_scale, float add_host_scale,
                                     float* out_grad, void* stream_)
{
    Levels lv;
    int rc = tree_ce_levels("loss_tree_ce_grad", K, H, W, num_levels, level_sizes, level_weight, &lv);
    if (rc != HSR_OK) return rc;
    if (!logits || !labels || !inv_count || !out_grad) {
        hsr_set_error("loss_tree_ce_grad: NULL logits / labels / inv_count / out_grad");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    launch_tree_ce_grad(H * W, K, lv, logits, labels, ignore_index, inv_count, upstream, add_grad, add_scale, add_host_scale, out_grad,
                        (hipStream_t)stream_);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_loss_leaf_mlp_ce(int K, int C, int H, int W, const float* sem, const float* weight, const float* bias,
                                    const int64_t* labels, int ignore_index, float* out_loss, float* d_sem, float* d_weight,
                                    float* d_bias, char* scratch, size_t scratch_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (K < 1 || K > LM_KP - 1 || C < 1 || C > 16 * LM_MAX_CT) {
        hsr_set_error("loss_leaf_mlp_ce: supports 1 <= K <= %d input channels and 1 <= C <= %d classes (got K=%d C=%d)", LM_KP - 1,
                      16 * LM_MAX_CT, K, C);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (hsr_bad_frame_size(H, W) || !sem || !weight || !bias || !labels || !out_loss) {
        hsr_set_error("loss_leaf_mlp_ce: invalid sizes H=%d W=%d or NULL sem/weight/bias/labels/out_loss", H, W);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const int N = H * W;
    const int CT = (C + 15) / 16;
    int nblk = (N + 255) / 256;
    if (nblk > LM_MAX_BLOCKS) nblk = LM_MAX_BLOCKS;
    // scratch: packed weights [CT*16][32] | inv count | loss partials | dW partials [nblk][CT*16*32]
    const size_t wt_bytes = hsr_align256((size_t)CT * 16 * LM_KP * sizeof(float));
    const size_t loss_bytes = hsr_align256((size_t)nblk * sizeof(float));
    const size_t dw_bytes = (size_t)nblk * CT * 16 * LM_KP * sizeof(float);
    int rc = hsr_check_scratch("loss_leaf_mlp_ce", scratch, scratch_bytes, wt_bytes + 256 + loss_bytes + dw_bytes);
    if (rc != HSR_OK) return rc;
    float* wt = reinterpret_cast<float*>(scratch);
    float* inv = reinterpret_cast<float*>(scratch + wt_bytes);
    float* part_loss = reinterpret_cast<float*>(scratch + wt_bytes + 256);
    float* part_dw = reinterpret_cast<float*>(scratch + wt_bytes + 256 + loss_bytes);
    leaf_pack_weights_kernel<<<(CT * 16 * LM_KP + 255) / 256, 256, 0, stream>>>(weight, bias, K, C, CT * 16, wt);
    valid_label_count_kernel<<<(N + LB - 1) / LB, LB, 0, stream>>>(labels, N, ignore_index, reinterpret_cast<unsigned*>(part_dw));
    count_finish_kernel<<<1, LB, 0, stream>>>(reinterpret_cast<unsigned*>(part_dw), (N + LB - 1) / LB, 1, 1, inv);
    const int ku = (K + 1 + 3) & ~3;
#define HSR_LEAF_LAUNCH(KU_, MC_) leaf_mlp_ce_kernel<KU_, MC_><<<nblk, 256, 0, stream>>>(sem, wt, labels, N, K, C, CT, ignore_index, inv, d_sem, part_loss, part_dw)
    if (CT <= 3) {         // <= 48 classes (NYU40 + void)
        if (ku <= 20) HSR_LEAF_LAUNCH(20, 3); else if (ku <= 28) HSR_LEAF_LAUNCH(28, 3); else HSR_LEAF_LAUNCH(32, 3);
    } else if (CT <= 7) {  // <= 112 classes (Replica)
        if (ku <= 20) HSR_LEAF_LAUNCH(20, 7); else if (ku <= 28) HSR_LEAF_LAUNCH(28, 7); else HSR_LEAF_LAUNCH(32, 7);
    } else {
        if (ku <= 20) HSR_LEAF_LAUNCH(20, 8); else if (ku <= 28) HSR_LEAF_LAUNCH(28, 8); else HSR_LEAF_LAUNCH(32, 8);
    }
#undef HSR_LEAF_LAUNCH
    finish_kernel<<<1, LB, 0, stream>>>(part_loss, nblk, 1, 1, inv, 1.0f, out_loss);
    if (d_weight || d_bias)
        leaf_finish_dw_kernel<<<(CT * 16 * LM_KP + 31) / 32, LFD_T, 0, stream>>>(part_dw, nblk, CT * 16 * LM_KP, K, C, d_weight, d_bias);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}
