// hsr_msssim.hip — multi-scale SSIM of one evaluated frame (gfx950); include/ext/hsr_msssim.h states the definition.
//
// What it replaces in the reference (utils/eval_helpers.py:722, :946, :1272): two masked copies of the image, two device->host copies
// (.cpu()) and pytorch_msssim.ms_ssim on the host's thread pool: per scale five grouped 11x1 and five 1x11 convolutions, the two
// maps, their means and two average pools.  Here:
//   * scale_kernel, one launch per scale, grid (tiles_x, tiles_y, 3 channels): a 32x32 tile of the filtered map needs 42x42 pixels of
//     both images in LDS (at scale 0 multiplied by the masks while they are loaded); the valid 11-tap filter runs as a horizontal pass
//     into LDS and a vertical pass out of it for x, y, xx, yy, xy, both sliding a 14-value register window over 4 outputs; cs and
//     ssim are formed in registers and summed per block (double; lanes, then waves, in a fixed order) into one partial pair per tile.
//     The same LDS tile yields the 2x2-pooled pixels of the next scale: each pooled pixel belongs to the one tile that owns the first
//     in-image row and column of its window (a tile owns the 32 rows / columns it starts at, the last one everything to the edge),
//     and the second row / column lies within that tile's 10-pixel halo.  No separate pooling pass, no masked copy;
//   * finish_kernel, one block: per scale the partial pairs in double, fixed order, then the means, relu, the weighted product and
//     the channel mean.
// 6 launches per frame.  Compiled with -ffp-contract=off: the value is pinned against restatements that evaluate
// E[xx] - mu*mu and its siblings as written; a multiply-add contracted into the variance (mu*mu exact inside the FMA, E[xx]
// rounded) changes the cancellation and with it the low-contrast pixels' cs, so every product and sum rounds once, in the order
// written.
#include "hsr_common.h"
#include "hsr_block.h"
#include "../../include/ext/hsr_msssim.h"
#include <cmath>

namespace {

constexpr int MB = 256;                  // threads per block
constexpr int MS_T = 32;                 // tile: outputs per side
constexpr int MS_E = MS_T + 10;          // tile: inputs per side
constexpr int MS_P = MS_E / 2 + 1;       // pooled candidates per side of a tile (the last tile owns up to 42 rows / columns)
constexpr int NS = HSR_EVAL_MSSSIM_SCALES;

struct Levels {
    int h[NS], w[NS];
    int tiles[NS];               // tiles_x * tiles_y
    long long pyr[NS];           // float offset of level s (s >= 1) in the pyramid: x planes [3][h][w], then y planes
    long long part[NS];          // double offset of the scale's partials [tile][channel][cs, ssim]
    long long pyr_floats, part_doubles;
};

bool bad_size(int H, int W)
{
    return H < HSR_EVAL_MSSSIM_MIN_SIDE || W < HSR_EVAL_MSSSIM_MIN_SIDE || hsr_bad_frame_size(H, W);
}

Levels levels_of(int H, int W)
{
    Levels lv{};
    long long pyr = 0, part = 0;
    for (int s = 0; s < NS; s++) {
        lv.h[s] = s ? (lv.h[s - 1] + 1) / 2 : H;      // floor((h + 2 (h % 2) - 2) / 2) + 1
        lv.w[s] = s ? (lv.w[s - 1] + 1) / 2 : W;
        lv.tiles[s] = ((lv.w[s] - 10 + MS_T - 1) / MS_T) * ((lv.h[s] - 10 + MS_T - 1) / MS_T);
        lv.pyr[s] = pyr;
        if (s) pyr += 6LL * lv.h[s] * lv.w[s];
        lv.part[s] = part;
        part += 6LL * lv.tiles[s];
    }
    lv.pyr_floats = pyr;
    lv.part_doubles = part;
    return lv;
}

// 4 consecutive outputs of the 11-tap filter from a 14-value window, taps in index order, one rounding per product and per sum
template <int NQ>
__device__ __forceinline__ void blur4(const float (&v)[NQ][14], const hsr_gauss& gw, float (&out)[NQ][4])
{
#pragma unroll
    for (int q = 0; q < NQ; q++)
#pragma unroll
        for (int o = 0; o < 4; o++) {
            float acc = gw.g[0] * v[q][o];
#pragma unroll
            for (int k = 1; k < 11; k++) acc = acc + gw.g[k] * v[q][o + k];
            out[q][o] = acc;
        }
}

struct ScaleArgs {
    const float* x;          // [3][h][w]: im (scale 0) or the level's x planes
    const float* y;
    const float* gt_depth;   // scale 0 only
    const float* opac;       // scale 0 only, may be NULL
    float sil_thres;
    int h, w;                // this scale
    float* nx;               // next level's planes [3][h2][w2], NULL at the last scale
    float* ny;
    int h2, w2;
    double* partials;        // [tile][3][2]
};

// grid (tiles_x, tiles_y, 3); block 256
template <bool FIRST>
__global__ __launch_bounds__(MB) void scale_kernel(ScaleArgs a, hsr_gauss gw)
{
    __shared__ float s_x[MS_E][MS_E + 1], s_y[MS_E][MS_E + 1];
    __shared__ float s_h[5][MS_E][MS_T + 1];   // horizontally filtered x, y, xx, yy, xy
    __shared__ double s_red[MB / 64][2];
    const int h = a.h, w = a.w, ch = blockIdx.z;
    const size_t plane = (size_t)ch * h * w;
    const int x0 = blockIdx.x * MS_T, y0 = blockIdx.y * MS_T;
    for (int i = threadIdx.x; i < MS_E * MS_E; i += MB) {
        const int ly = i / MS_E, lx = i - ly * MS_E;
        const int gx = x0 + lx, gy = y0 + ly;
        const bool in = gx < w && gy < h;       // beyond the image: zeros, which reach no output inside the map
        const size_t p = (size_t)(in ? gy : 0) * w + (in ? gx : 0);
        float xv = a.x[plane + p], yv = a.y[plane + p];
        if (FIRST) {
            // the reference's products, in its order: im * presence * valid (presence only in the silhouette branch)
            const float valid = a.gt_depth[p] > 0.f ? 1.f : 0.f;
            if (a.opac) {
                const float pres = a.opac[p] > a.sil_thres ? 1.f : 0.f;
                xv = xv * pres;
                yv = yv * pres;
            }
            xv = xv * valid;
            yv = yv * valid;
        }
        s_x[ly][lx] = in ? xv : 0.f;
        s_y[ly][lx] = in ? yv : 0.f;
    }
    __syncthreads();

    // the next scale's pixels of this channel: 2x2 average, zero padding of (size % 2) in front, divisor 4
    if (a.nx) {
        const int py_pad = h & 1, px_pad = w & 1;
        const int y1 = blockIdx.y + 1 == gridDim.y ? h : y0 + MS_T, x1 = blockIdx.x + 1 == gridDim.x ? w : x0 + MS_T;   // owned: [y0, y1) x [x0, x1)
        const size_t plane2 = (size_t)ch * a.h2 * a.w2;
        for (int i = threadIdx.x; i < MS_P * MS_P; i += MB) {
            const int py = y0 / 2 + i / MS_P, px = x0 / 2 + i % MS_P;
            const int ry = 2 * py - py_pad, rx = 2 * px - px_pad;        // first row / column of the window; -1 is padding
            const int ay = ry < 0 ? 0 : ry, ax = rx < 0 ? 0 : rx;
            if (py >= a.h2 || px >= a.w2 || ay < y0 || ay >= y1 || ax < x0 || ax >= x1) continue;
            // rows ry, ry + 1 <= h - 1 and columns rx, rx + 1 <= w - 1 lie inside the 42 x 42 tile: see the file header
            const int l0 = ry - y0, c0 = rx - x0;
            const bool top = ry >= 0, left = rx >= 0;
            const float x00 = top && left ? s_x[l0][c0] : 0.f, x01 = top ? s_x[l0][c0 + 1] : 0.f;
            const float x10 = left ? s_x[l0 + 1][c0] : 0.f, x11 = s_x[l0 + 1][c0 + 1];
            const float y00 = top && left ? s_y[l0][c0] : 0.f, y01 = top ? s_y[l0][c0 + 1] : 0.f;
            const float y10 = left ? s_y[l0 + 1][c0] : 0.f, y11 = s_y[l0 + 1][c0 + 1];
            const size_t o = plane2 + (size_t)py * a.w2 + px;
            a.nx[o] = (((x00 + x01) + x10) + x11) * 0.25f;
            a.ny[o] = (((y00 + y01) + y10) + y11) * 0.25f;
        }
    }

    // pass 1: rows 0..41, 8 groups of 4 columns each
    for (int item = threadIdx.x; item < MS_E * (MS_T / 4); item += MB) {
        const int r = item / (MS_T / 4), c0 = (item % (MS_T / 4)) * 4;
        float v[5][14];
#pragma unroll
        for (int k = 0; k < 14; k++) {
            const float xa = s_x[r][c0 + k], yb = s_y[r][c0 + k];
            v[0][k] = xa; v[1][k] = yb; v[2][k] = xa * xa; v[3][k] = yb * yb; v[4][k] = xa * yb;
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
    const float c1 = (float)(0.01 * 0.01), c2 = (float)(0.03 * 0.03);
    double acc_cs = 0.0, acc_ss = 0.0;
    const int ox = x0 + col;
#pragma unroll
    for (int o = 0; o < 4; o++) {
        const int oy = y0 + r0 + o;
        const float m1 = m[0][o], m2 = m[1][o];
        const float mu1_sq = m1 * m1, mu2_sq = m2 * m2, mu12 = m1 * m2;
        const float sig1 = m[2][o] - mu1_sq, sig2 = m[3][o] - mu2_sq, sig12 = m[4][o] - mu12;
        const float cs = (2.f * sig12 + c2) / (sig1 + sig2 + c2);
        const float ss = (2.f * mu12 + c1) / (mu1_sq + mu2_sq + c1) * cs;
        const bool live = ox < w - 10 && oy < h - 10;
        acc_cs += live ? (double)cs : 0.0;
        acc_ss += live ? (double)ss : 0.0;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    acc_cs = hsr_wave_sum(acc_cs);
    acc_ss = hsr_wave_sum(acc_ss);
    if (lane == 0) { s_red[wv][0] = acc_cs; s_red[wv][1] = acc_ss; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        a.partials[(tile * 3 + ch) * 2 + k] = ((s_red[0][k] + s_red[1][k]) + s_red[2][k]) + s_red[3][k];
    }
}

__global__ __launch_bounds__(MB) void finish_kernel(const double* __restrict__ partials, Levels lv, double* __restrict__ out)
{
    __shared__ double s_acc[6][MB];
    __shared__ double s_mean[NS][6];      // [scale][channel * 2 + {cs, ssim}]
    for (int s = 0; s < NS; s++) {
        const double* __restrict__ p = partials + lv.part[s];
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int t = threadIdx.x; t < lv.tiles[s]; t += MB)
#pragma unroll
            for (int k = 0; k < 6; k++) acc[k] += p[(size_t)t * 6 + k];
#pragma unroll
        for (int k = 0; k < 6; k++) s_acc[k][threadIdx.x] = acc[k];
        __syncthreads();
        for (int o = MB / 2; o > 0; o >>= 1) {
            if (threadIdx.x < o)
#pragma unroll
                for (int k = 0; k < 6; k++) s_acc[k][threadIdx.x] += s_acc[k][threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x < 6) s_mean[s][threadIdx.x] = s_acc[threadIdx.x][0] / ((double)(lv.h[s] - 10) * (double)(lv.w[s] - 10));
        __syncthreads();
    }
    if (threadIdx.x < NS * 6) out[1 + threadIdx.x] = s_mean[threadIdx.x / 6][threadIdx.x % 6];
    if (threadIdx.x == 0) {
        const double weight[NS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
        double score = 0.0;
        for (int c = 0; c < 3; c++) {
            double prod = 1.0;
            for (int s = 0; s < NS; s++) {
                const double v = s_mean[s][c * 2 + (s == NS - 1 ? 1 : 0)];
                prod *= pow(v > 0.0 ? v : 0.0, weight[s]);
            }
            score += prod;
        }
        out[0] = score / 3.0;
    }
}

}  // namespace

// ---------------------------------------------------------------- C ABI
extern "C" size_t hsr_eval_msssim_scratch_bytes(int H, int W)
{
    if (bad_size(H, W)) return 1024;
    const Levels lv = levels_of(H, W);
    return hsr_align256((size_t)lv.pyr_floats * sizeof(float)) + hsr_align256((size_t)lv.part_doubles * sizeof(double));
}

extern "C" int hsr_eval_msssim(int H, int W, const float* im, const float* gt_im, const float* gt_depth, const float* final_opacity,
                               float sil_thres, double* out, char* scratch, size_t scratch_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (bad_size(H, W) || !im || !gt_im || !gt_depth || !out) {
        hsr_set_error("eval_msssim: invalid size H=%d W=%d (both sides >= %d: the smaller side must exceed 160 for the 4 downsamplings) "
                      "or NULL im / gt_im / gt_depth / out", H, W, HSR_EVAL_MSSSIM_MIN_SIDE);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (int rc = hsr_check_scratch("eval_msssim", scratch, scratch_bytes, hsr_eval_msssim_scratch_bytes(H, W))) return rc;
    const Levels lv = levels_of(H, W);
    float* pyr = reinterpret_cast<float*>(scratch);
    double* partials = reinterpret_cast<double*>(scratch + hsr_align256((size_t)lv.pyr_floats * sizeof(float)));
    const hsr_gauss gw = hsr_gauss_window();
    for (int s = 0; s < NS; s++) {
        ScaleArgs a{};
        a.h = lv.h[s];
        a.w = lv.w[s];
        const size_t n = (size_t)a.h * a.w;
        a.x = s ? pyr + lv.pyr[s] : im;
        a.y = s ? pyr + lv.pyr[s] + 3 * n : gt_im;
        a.gt_depth = gt_depth;
        a.opac = final_opacity;
        a.sil_thres = sil_thres;
        if (s + 1 < NS) {
            a.h2 = lv.h[s + 1];
            a.w2 = lv.w[s + 1];
            a.nx = pyr + lv.pyr[s + 1];
            a.ny = a.nx + 3 * (size_t)a.h2 * a.w2;
        }
        a.partials = partials + lv.part[s];
        const dim3 grid((a.w - 10 + MS_T - 1) / MS_T, (a.h - 10 + MS_T - 1) / MS_T, 3);
        if (s == 0) scale_kernel<true><<<grid, MB, 0, stream>>>(a, gw);
        else scale_kernel<false><<<grid, MB, 0, stream>>>(a, gw);
    }
    finish_kernel<<<1, MB, 0, stream>>>(partials, lv, out);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}
