// hsr_frame_ingest.hip — device ingest of one raw sensor frame to one, two or three sizes (gfx950), DESIGN.md §7 row 8.
// See include/ext/hsr_frame_ingest.h for the three rules, step by step, and the reference lines (basedataset.py:223-227, :248-256,
// replica.py:241-299, scripts/hierslam.py:1777), and include/ext/hsr_frame_ingest_planes.h for the same rules with a source size per
// image and a leaf column in the label table (scannet.py:284-339).  ONE kernel runs behind both entries: hsr_frame_ingest passes the
// sensor size three times and leaf_column = 0.
//   ingest_kernel : one thread per destination pixel over the concatenated pixel ranges of the levels (level 0's pixels first): the
//                   three colour channels bilinearly in float64 from four interleaved 8-bit taps, then / 255; the depth from one raw
//                   source word divided by the scale; at level 0 the L + 1 int64 label planes from one raw id and its table row.
// Memory-bound and small (a 1200x680 frame to itself and two 600x340 levels reads 8 MB and writes 20 MB with 5-level labels); no
// reuse worth staging in LDS.  Compiled with -ffp-contract=off: the three float64 lerps are evaluated as the header writes them.
#include <math.h>

#include "hsr_common.h"
#include "hsr_ingest_expr.h"
#include "../../include/hsr_eval.h"
#include "../../include/ext/hsr_frame_resample.h"
#include "../../include/ext/hsr_frame_ingest.h"
#include "../../include/ext/hsr_frame_ingest_planes.h"

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

// table: int32 [n_ids, L + leaf], leaf 0 or 1; n_ids 0 without a table (no id is then "known" and the table is not read)
template <int DT>
__global__ __launch_bounds__(IB) void ingest_kernel(const uint8_t* __restrict__ color, const void* __restrict__ depth, Sources src,
                                                    double depth_scale, const int* __restrict__ labels, int L, int leaf,
                                                    const int* __restrict__ table, int n_ids, Levels lv, long long n_all,
                                                    long long* __restrict__ out_labels)
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

// the checks and the launch of both entries; `planes`: hsr_frame_ingest_planes (the messages name the entry and its arguments)
int ingest(bool planes, Sources src, const uint8_t* color_u8, const void* depth_raw, int depth_type, double depth_scale,
           const int* labels, int num_levels, const int* table, int n_ids, int leaf_column,
           int n_out, const hsr_ingest_level* levels, int64_t* out_labels, hipStream_t stream)
{
    const char* who = planes ? "frame_ingest_planes" : "frame_ingest";
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
            hsr_set_error("frame_ingest: sides must be 1..%d: sensor %dx%d, level 0 %dx%d (of %d levels)", HSR_RESAMPLE_MAX_SIDE, src.Hc,
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
            hsr_set_error("frame_ingest: num_levels must be 0..%d, and with num_levels > 0 a tree_table of n_ids >= 1 rows; got %d levels, "
                          "n_ids %d", HSR_EVAL_MAX_LEVELS, num_levels, n_ids);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    bool null = !color_u8 || !depth_raw || ((labels == nullptr) != (out_labels == nullptr));
    for (int k = 0; k < n_out; k++) null = null || !levels[k].color || !levels[k].depth;
    if (null) {
        hsr_set_error("%s: NULL color_u8 / depth_raw, a NULL output of a requested level, or labels without out_labels (or the reverse)", who);
        return HSR_ERR_INVALID_ARGUMENT;
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
#define HSR_INGEST_LAUNCH(DT) \
    ingest_kernel<DT><<<nblk, IB, 0, stream>>>(color_u8, depth_raw, src, depth_scale, labels, num_levels, leaf_column, table, n_ids_k, lv, n_all, ol)
    if (depth_type == HSR_INGEST_DEPTH_U16) HSR_INGEST_LAUNCH(HSR_INGEST_DEPTH_U16);
    else if (depth_type == HSR_INGEST_DEPTH_I32) HSR_INGEST_LAUNCH(HSR_INGEST_DEPTH_I32);
    else HSR_INGEST_LAUNCH(HSR_INGEST_DEPTH_F32);
#undef HSR_INGEST_LAUNCH
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

}  // namespace

extern "C" int hsr_frame_ingest(int Hs, int Ws, const uint8_t* color_u8, const void* depth_raw, int depth_type, double depth_scale,
                                const int* labels, int num_levels, const int* tree_table, int n_ids,
                                int n_out, const hsr_ingest_level* levels, int64_t* out_labels, void* stream_)
{
    return ingest(false, Sources{Hs, Ws, Hs, Ws, Hs, Ws}, color_u8, depth_raw, depth_type, depth_scale, labels, num_levels, tree_table, n_ids,
                  0, n_out, levels, out_labels, (hipStream_t)stream_);
}

extern "C" int hsr_frame_ingest_planes(int Hc, int Wc, const uint8_t* color_u8,
                                       int Hd, int Wd, const void* depth_raw, int depth_type, double depth_scale,
                                       int Hl, int Wl, const int* labels,
                                       int num_levels, const int* label_table, int n_ids, int leaf_column,
                                       int n_out, const hsr_ingest_level* levels, int64_t* out_labels, void* stream_)
{
    return ingest(true, Sources{Hc, Wc, Hd, Wd, Hl, Wl}, color_u8, depth_raw, depth_type, depth_scale, labels, num_levels, label_table, n_ids,
                  leaf_column, n_out, levels, out_labels, (hipStream_t)stream_);
}
