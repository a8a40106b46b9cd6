// hsr_frame_ingest.hip — device ingest of one raw sensor frame to one, two or three sizes (gfx950), DESIGN.md §7 row 8.
// See include/ext/hsr_frame_ingest.h for the three rules, step by step, and the reference lines (basedataset.py:223-227, :248-256,
// replica.py:241-299, scripts/hierslam.py:1777), and include/ext/hsr_frame_ingest_planes.h for the same rules with a source size per
// image and a leaf column in the label table (scannet.py:284-339), and include/sensor/hsr_frame_undistort.h for hsr_frame_ingest with the
// colour image undistorted on the way (basedataset.py:306-309).  ONE kernel runs behind all three entries: hsr_frame_ingest passes the
// sensor size three times and leaf_column = 0; hsr_frame_ingest_undistort does the same and sets the compile-time flag UND, with which
// a colour tap is a value of the undistorted image U at that pixel instead of the 8-bit pixel.
//   ingest_kernel : one thread per destination pixel over the concatenated pixel ranges of the levels (level 0's pixels first): the
//                   three colour channels bilinearly in float64 from four interleaved 8-bit taps, then / 255; the depth from one raw
//                   source word divided by the scale; at level 0 the L + 1 int64 label planes from one raw id and its table row.
//                   With UND each of the four taps is U: the pixel's source coordinates in float64, quantised to 1/32 pixel, and the
//                   exact integer blend of four 8-bit taps that are 0 outside the image (one tap at a level of the sensor's size).
// Memory-bound and small (a 1200x680 frame to itself and two 600x340 levels reads 8 MB and writes 20 MB with 5-level labels); no
// reuse worth staging in LDS.  Compiled with -ffp-contract=off: the three float64 lerps are evaluated as the header writes them.
#include <math.h>

#include "hsr_common.h"
#include "hsr_ingest_expr.h"
#include "../../include/hsr_eval.h"
#include "../../include/ext/hsr_frame_resample.h"
#include "../../include/ext/hsr_frame_ingest.h"
#include "../../include/ext/hsr_frame_ingest_planes.h"
#include "../../include/sensor/hsr_frame_undistort.h"

namespace {

constexpr int IB = 256;

struct Levels {
    hsr_ingest_level l[HSR_INGEST_MAX_LEVELS];
    long long end[HSR_INGEST_MAX_LEVELS];      // prefix sums of H * W: level k owns [end[k-1], end[k])
};

// the three source images: colour [Hc,Wc,3], depth [Hd,Wd], labels [Hl,Wl] (1x1 and never read without labels)
struct Sources {
    int Hc, Wc, Hd, Wd, Hl, Wl;
};

template <int DT>
__device__ __forceinline__ double raw_depth(const void* __restrict__ p, size_t i)
{
    if (DT == HSR_INGEST_DEPTH_U16) return (double)static_cast<const uint16_t*>(p)[i];
    if (DT == HSR_INGEST_DEPTH_I32) return (double)static_cast<const int32_t*>(p)[i];
    return (double)static_cast<const float*>(p)[i];
}

// where the undistorted pixel (u, v) reads the 8-bit image: the tap (sy, sx), the weights ax, ay / 32 of the taps after it
// (include/sensor/hsr_frame_undistort.h, U); !ok: a NaN coordinate, the pixel is 0
struct Und {
    int sx, sy, ax, ay;
    bool ok;
};

__device__ __forceinline__ Und und_at(int u, int v, const hsr_lens& lens)
{
    double us, vs;
    hsr_undistort_source(u, v, lens, us, vs);      // hsr_ingest_expr.h, in double
    Und t;
    const bool okx = hsr_undistort_step(us, t.sx, t.ax), oky = hsr_undistort_step(vs, t.sy, t.ay);
    t.ok = okx && oky;
    return t;
}

// U[v][u][ch] of the pixel `t` was made for: an exact integer below 2^18 over 1024; a tap outside the image is 0 and is not read
__device__ __forceinline__ double und_value(const uint8_t* __restrict__ color, int Hc, int Wc, const Und& t, int ch)
{
    if (!t.ok) return 0.0;
    const bool x0 = t.sx >= 0 && t.sx < Wc, x1 = t.sx + 1 >= 0 && t.sx + 1 < Wc;      // |sx|, |sy| <= 2^25
    const bool y0 = t.sy >= 0 && t.sy < Hc, y1 = t.sy + 1 >= 0 && t.sy + 1 < Hc;
    const uint8_t* __restrict__ p = color + ((long long)t.sy * Wc + t.sx) * 3 + ch;      // followed only where the tap is inside
    const int a = y0 && x0 ? p[0] : 0, b = y0 && x1 ? p[3] : 0;
    const int c = y1 && x0 ? p[(size_t)Wc * 3] : 0, d = y1 && x1 ? p[(size_t)Wc * 3 + 3] : 0;
    const int n = a * (32 - t.ax) * (32 - t.ay) + b * t.ax * (32 - t.ay) + c * (32 - t.ax) * t.ay + d * t.ax * t.ay;
    return (double)n / 1024.0;
}

// table: int32 [n_ids, L + leaf], leaf 0 or 1; n_ids 0 without a table (no id is then "known" and the table is not read)
// UND: a colour tap is U at that pixel (lens: the sensor's camera and coefficients), else the 8-bit pixel (lens is not read)
template <int DT, bool UND>
__global__ __launch_bounds__(IB) void ingest_kernel(const uint8_t* __restrict__ color, const void* __restrict__ depth, Sources src,
                                                    double depth_scale, const int* __restrict__ labels, int L, int leaf,
                                                    const int* __restrict__ table, int n_ids, Levels lv, long long n_all,
                                                    long long* __restrict__ out_labels, hsr_lens lens)
{
    long long i = (long long)blockIdx.x * IB + threadIdx.x;
    if (i >= n_all) return;
    const int k = (i >= lv.end[0]) + (i >= lv.end[1]);      // an absent level ends where the last one does: never selected
    i -= k == 0 ? 0 : k == 1 ? lv.end[0] : lv.end[1];
    // selected with constant indices: a dynamically indexed by-value struct would go through scratch memory
    const int Hd = k == 0 ? lv.l[0].H : k == 1 ? lv.l[1].H : lv.l[2].H;
    const int Wd = k == 0 ? lv.l[0].W : k == 1 ? lv.l[1].W : lv.l[2].W;
    float* __restrict__ oc = k == 0 ? lv.l[0].color : k == 1 ? lv.l[1].color : lv.l[2].color;
    float* __restrict__ od = k == 0 ? lv.l[0].depth : k == 1 ? lv.l[1].depth : lv.l[2].depth;
    const int y = (int)(i / Wd), x = (int)(i - (long long)y * Wd);      // i < Hd * Wd
    int x0, x1, y0, y1;
    double fx, fy;
    hsr_taps(x, src.Wc, Wd, x0, x1, fx);      // hsr_ingest_expr.h, in double
    hsr_taps(y, src.Hc, Hd, y0, y1, fy);
    const size_t dplane = (size_t)Hd * Wd;
    if constexpr (!UND) {
        const uint8_t* __restrict__ r0 = color + (size_t)y0 * src.Wc * 3;
        const uint8_t* __restrict__ r1 = color + (size_t)y1 * src.Wc * 3;
        const size_t c0 = (size_t)x0 * 3, c1 = (size_t)x1 * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const double a = (double)r0[c0 + ch], b = (double)r0[c1 + ch], c = (double)r1[c0 + ch], d = (double)r1[c1 + ch];
            const double top = a + fx * (b - a);
            const double bot = c + fx * (d - c);
            const double v = top + fy * (bot - top);
            oc[ch * dplane + (size_t)i] = hsr_ingest_colour((float)v);      // float(v) / 255.0f (hsr_ingest_expr.h)
        }
    } else if (Hd == src.Hc && Wd == src.Wc) {
        // a level of the sensor's size: x0 = x, y0 = y and both weights are 0, so v = a + 0 * (b - a) is a bit for bit; one tap
        const Und ta = und_at(x, y, lens);
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
            oc[ch * dplane + (size_t)i] = hsr_ingest_colour((float)und_value(color, src.Hc, src.Wc, ta, ch));
    } else {
        const Und ta = und_at(x0, y0, lens), tb = und_at(x1, y0, lens), tc = und_at(x0, y1, lens), td = und_at(x1, y1, lens);
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const double a = und_value(color, src.Hc, src.Wc, ta, ch), b = und_value(color, src.Hc, src.Wc, tb, ch);
            const double c = und_value(color, src.Hc, src.Wc, tc, ch), d = und_value(color, src.Hc, src.Wc, td, ch);
            const double top = a + fx * (b - a);
            const double bot = c + fx * (d - c);
            const double v = top + fy * (bot - top);
            oc[ch * dplane + (size_t)i] = hsr_ingest_colour((float)v);
        }
    }
    // nearest, each image from its own size: products < 2^28; xs <= W_src - 1, ys <= H_src - 1
    const size_t sd = (size_t)((y * src.Hd) / Hd) * src.Wd + (x * src.Wd) / Wd;
    od[i] = hsr_ingest_depth(raw_depth<DT>(depth, sd), depth_scale);
    if (k == 0 && out_labels) {
        const size_t sl = (size_t)((y * src.Hl) / Hd) * src.Wl + (x * src.Wl) / Wd;
        const int id = labels[sl];
        const bool known = id >= 0 && id < n_ids;
        const int* __restrict__ row = table + (size_t)(known ? id : 0) * (L + leaf);      // not read unless known (and L + leaf > 0)
        for (int l = 0; l < L; l++)
            out_labels[l * dplane + (size_t)i] = known ? row[l] : id;
        out_labels[L * dplane + (size_t)i] = (leaf && known) ? row[L] : id;
    }
}

// the checks and the launch of the three entries; `planes`: hsr_frame_ingest_planes (the messages name the entry and its arguments);
// `lens`: hsr_frame_ingest_undistort, else NULL
int ingest(bool planes, const hsr_lens* lens, Sources src, const uint8_t* color_u8, const void* depth_raw, int depth_type, double depth_scale,
           const int* labels, int num_levels, const int* table, int n_ids, int leaf_column,
           int n_out, const hsr_ingest_level* levels, int64_t* out_labels, hipStream_t stream)
{
    const char* who = planes ? "frame_ingest_planes" : lens ? "frame_ingest_undistort" : "frame_ingest";
    if (n_out < 1 || n_out > HSR_INGEST_MAX_LEVELS || !levels) {
        hsr_set_error("%s: n_out must be 1..%d with a host array of that many levels; got %d", who, HSR_INGEST_MAX_LEVELS, n_out);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    bool sides = hsr_side_ok(src.Hc) && hsr_side_ok(src.Wc) && hsr_side_ok(src.Hd) && hsr_side_ok(src.Wd) &&
                 (!labels || (hsr_side_ok(src.Hl) && hsr_side_ok(src.Wl)));
    for (int k = 0; k < n_out; k++) sides = sides && hsr_side_ok(levels[k].H) && hsr_side_ok(levels[k].W);
    if (!sides) {
        if (planes)
            hsr_set_error("frame_ingest_planes: sides must be 1..%d: colour %dx%d, depth %dx%d, labels %dx%d (checked when given), "
                          "level 0 %dx%d (of %d levels)", HSR_RESAMPLE_MAX_SIDE, src.Hc, src.Wc, src.Hd, src.Wd, src.Hl, src.Wl,
                          levels[0].H, levels[0].W, n_out);
        else
            hsr_set_error("%s: sides must be 1..%d: sensor %dx%d, level 0 %dx%d (of %d levels)", who, HSR_RESAMPLE_MAX_SIDE, src.Hc,
                          src.Wc, levels[0].H, levels[0].W, n_out);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (depth_type != HSR_INGEST_DEPTH_U16 && depth_type != HSR_INGEST_DEPTH_I32 && depth_type != HSR_INGEST_DEPTH_F32) {
        hsr_set_error("%s: depth_type must be HSR_INGEST_DEPTH_U16, _I32 or _F32; got %d", who, depth_type);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!isfinite(depth_scale) || depth_scale == 0.0) {
        hsr_set_error("%s: depth_scale must be finite and non-zero; got %g", who, depth_scale);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const bool has_table = num_levels > 0 || leaf_column == 1;
    if (num_levels < 0 || num_levels > HSR_EVAL_MAX_LEVELS || (leaf_column != 0 && leaf_column != 1) || (has_table && (!table || n_ids < 1))) {
        if (planes)
            hsr_set_error("frame_ingest_planes: num_levels must be 0..%d, leaf_column 0 or 1, and with num_levels > 0 or leaf_column a "
                          "label_table of n_ids >= 1 rows; got %d levels, leaf_column %d, n_ids %d", HSR_EVAL_MAX_LEVELS, num_levels,
                          leaf_column, n_ids);
        else
            hsr_set_error("%s: num_levels must be 0..%d, and with num_levels > 0 a tree_table of n_ids >= 1 rows; got %d levels, "
                          "n_ids %d", who, HSR_EVAL_MAX_LEVELS, num_levels, n_ids);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    bool null = !color_u8 || !depth_raw || ((labels == nullptr) != (out_labels == nullptr));
    for (int k = 0; k < n_out; k++) null = null || !levels[k].color || !levels[k].depth;
    if (null) {
        hsr_set_error("%s: NULL color_u8 / depth_raw, a NULL output of a requested level, or labels without out_labels (or the reverse)", who);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (lens) {
        if (!isfinite(lens->fx) || !isfinite(lens->fy) || lens->fx == 0.0 || lens->fy == 0.0) {
            hsr_set_error("%s: fx and fy must be finite and non-zero; got %g, %g", who, lens->fx, lens->fy);
            return HSR_ERR_INVALID_ARGUMENT;
        }
        if (!isfinite(lens->cx) || !isfinite(lens->cy) || !isfinite(lens->k1) || !isfinite(lens->k2) || !isfinite(lens->p1) ||
            !isfinite(lens->p2) || !isfinite(lens->k3)) {
            hsr_set_error("%s: cx, cy and the coefficients k1, k2, p1, p2, k3 must be finite; got %g, %g and %g, %g, %g, %g, %g", who,
                          lens->cx, lens->cy, lens->k1, lens->k2, lens->p1, lens->p2, lens->k3);
            return HSR_ERR_INVALID_ARGUMENT;
        }
    }
    if (!labels) src.Hl = src.Wl = 1;      // not read by the kernel; never a side it was not checked for
    Levels lv{};
    long long n_all = 0;
    for (int k = 0; k < HSR_INGEST_MAX_LEVELS; k++) {
        if (k < n_out) {
            lv.l[k] = levels[k];
            n_all += (long long)levels[k].H * levels[k].W;      // <= 3 * 2^28
        } else {
            lv.l[k] = hsr_ingest_level{0, 1, nullptr, nullptr};
        }
        lv.end[k] = n_all;
    }
    const unsigned nblk = (unsigned)((n_all + IB - 1) / IB);
    long long* ol = reinterpret_cast<long long*>(out_labels);
    const int n_ids_k = has_table ? n_ids : 0;      // without a table no id is "known"
    const hsr_lens lens_k = lens ? *lens : hsr_lens{};      // read by the UND instantiations only
#define HSR_INGEST_ARGS color_u8, depth_raw, src, depth_scale, labels, num_levels, leaf_column, table, n_ids_k, lv, n_all, ol, lens_k
#define HSR_INGEST_LAUNCH(DT)                                                        \
    do {                                                                             \
        if (lens) ingest_kernel<DT, true><<<nblk, IB, 0, stream>>>(HSR_INGEST_ARGS); \
        else ingest_kernel<DT, false><<<nblk, IB, 0, stream>>>(HSR_INGEST_ARGS);     \
    } while (0)
    if (depth_type == HSR_INGEST_DEPTH_U16) HSR_INGEST_LAUNCH(HSR_INGEST_DEPTH_U16);
    else if (depth_type == HSR_INGEST_DEPTH_I32) HSR_INGEST_LAUNCH(HSR_INGEST_DEPTH_I32);
    else HSR_INGEST_LAUNCH(HSR_INGEST_DEPTH_F32);
#undef HSR_INGEST_LAUNCH
#undef HSR_INGEST_ARGS
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

}  // namespace

extern "C" int hsr_frame_ingest(int Hs, int Ws, const uint8_t* color_u8, const void* depth_raw, int depth_type, double depth_scale,
                                const int* labels, int num_levels, const int* tree_table, int n_ids,
                                int n_out, const hsr_ingest_level* levels, int64_t* out_labels, void* stream_)
{
    return ingest(false, nullptr, Sources{Hs, Ws, Hs, Ws, Hs, Ws}, color_u8, depth_raw, depth_type, depth_scale, labels, num_levels, tree_table, n_ids,
                  0, n_out, levels, out_labels, (hipStream_t)stream_);
}

extern "C" int hsr_frame_ingest_planes(int Hc, int Wc, const uint8_t* color_u8,
                                       int Hd, int Wd, const void* depth_raw, int depth_type, double depth_scale,
                                       int Hl, int Wl, const int* labels,
                                       int num_levels, const int* label_table, int n_ids, int leaf_column,
                                       int n_out, const hsr_ingest_level* levels, int64_t* out_labels, void* stream_)
{
    return ingest(true, nullptr, Sources{Hc, Wc, Hd, Wd, Hl, Wl}, color_u8, depth_raw, depth_type, depth_scale, labels, num_levels, label_table, n_ids,
                  leaf_column, n_out, levels, out_labels, (hipStream_t)stream_);
}

extern "C" int hsr_frame_ingest_undistort(int Hs, int Ws, const uint8_t* color_u8, const void* depth_raw, int depth_type, double depth_scale,
                                          const int* labels, int num_levels, const int* tree_table, int n_ids,
                                          double fx, double fy, double cx, double cy,
                                          double k1, double k2, double p1, double p2, double k3,
                                          int n_out, const hsr_ingest_level* levels, int64_t* out_labels, void* stream_)
{
    const hsr_lens lens{fx, fy, cx, cy, k1, k2, p1, p2, k3};
    return ingest(false, &lens, Sources{Hs, Ws, Hs, Ws, Hs, Ws}, color_u8, depth_raw, depth_type, depth_scale, labels, num_levels, tree_table,
                  n_ids, 0, n_out, levels, out_labels, (hipStream_t)stream_);
}
