// hsr_frame_resample.hip — device resample of one RGB-D frame to one or two sizes (gfx950), DESIGN.md §7 row 8.
// See include/ext/hsr_frame_resample.h for both rules, step by step, and the reference lines (basedataset.py:223-227, :248-252).
//   resample_kernel : one thread per destination pixel of either level (level 0's pixels first, then level 1's): the three colour
//                     channels bilinearly from four taps each, the depth by copying one source word.
// Memory-bound and small (a 1200x680 frame to two 600x340 levels reads 13 MB and writes 3 MB).  Compiled with -ffp-contract=off:
// the three lerps are evaluated as the header writes them, so that equal sizes copy and the result is comparable with a plain fp32
// restatement.
#include "hsr_common.h"
#include "hsr_ingest_expr.h"
#include "../../include/ext/hsr_frame_resample.h"

namespace {

constexpr int RB = 256;

struct Level { int H, W; float* color; float* depth; };

__global__ __launch_bounds__(RB) void resample_kernel(const float* __restrict__ color, const uint32_t* __restrict__ depth, int H, int W,
                                                      Level l0, Level l1, long long n0, long long n_all)
{
    long long i = (long long)blockIdx.x * RB + threadIdx.x;
    if (i >= n_all) return;
    const bool second = i >= n0;
    if (second) i -= n0;
    const int Hd = second ? l1.H : l0.H, Wd = second ? l1.W : l0.W;
    float* __restrict__ oc = second ? l1.color : l0.color;
    uint32_t* __restrict__ od = reinterpret_cast<uint32_t*>(second ? l1.depth : l0.depth);
    const int y = (int)(i / Wd), x = (int)(i - (long long)y * Wd);      // i < Hd * Wd
    int x0, x1, y0, y1;
    float fx, fy;
    hsr_taps(x, W, Wd, x0, x1, fx);      // hsr_ingest_expr.h, in float
    hsr_taps(y, H, Hd, y0, y1, fy);
    const size_t plane = (size_t)H * W, dplane = (size_t)Hd * Wd;
    const size_t r0 = (size_t)y0 * W, r1 = (size_t)y1 * W;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const float* __restrict__ s = color + ch * plane;
        const float a = s[r0 + x0], b = s[r0 + x1], c = s[r1 + x0], d = s[r1 + x1];
        const float top = a + fx * (b - a);
        const float bot = c + fx * (d - c);
        oc[ch * dplane + (size_t)i] = top + fy * (bot - top);
    }
    const int xs = (x * W) / Wd, ys = (y * H) / Hd;      // products < 2^28
    od[i] = depth[(size_t)ys * W + xs];
}

}  // namespace

extern "C" int hsr_frame_resample(int H, int W, const float* color, const float* depth, int H0, int W0, float* out_color0,
                                  float* out_depth0, int H1, int W1, float* out_color1, float* out_depth1, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!hsr_side_ok(H) || !hsr_side_ok(W) || !hsr_side_ok(H0) || !hsr_side_ok(W0) || (H1 != 0 && (!hsr_side_ok(H1) || !hsr_side_ok(W1)))) {
        hsr_set_error("frame_resample: sides must be 1..%d (H1 == 0 skips level 1): source %dx%d, level 0 %dx%d, level 1 %dx%d",
                      HSR_RESAMPLE_MAX_SIDE, H, W, H0, W0, H1, W1);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!color || !depth || !out_color0 || !out_depth0 || (H1 != 0 && (!out_color1 || !out_depth1))) {
        hsr_set_error("frame_resample: NULL color / depth or NULL output of a requested level");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const Level l0{H0, W0, out_color0, out_depth0};
    const Level l1 = H1 != 0 ? Level{H1, W1, out_color1, out_depth1} : Level{0, 1, nullptr, nullptr};
    const long long n0 = (long long)H0 * W0, n_all = n0 + (long long)l1.H * l1.W;      // <= 2^29
    const unsigned nblk = (unsigned)((n_all + RB - 1) / RB);
    resample_kernel<<<nblk, RB, 0, stream>>>(color, reinterpret_cast<const uint32_t*>(depth), H, W, l0, l1, n0, n_all);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}
