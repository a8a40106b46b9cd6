// hsr_common.h — shared declarations of the gfx950 rasterizer library (internal, not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#define HSR_TILE_X 16
#define HSR_TILE_Y 16
#define HSR_TILE_PIX 256
#define HSR_NUM_CHANNELS 3

// ---- opaque state, carved out of the caller's three byte buffers (all fields 256-B aligned) ----
// The reference keeps the same information in GeometryState / ImageState / BinningState
// (cuda_rasterizer/rasterizer_impl.h:29-64); the layout here is ours: ranges are per TILE (the
// reference reserves one per pixel, rasterizer_impl.cu:177), there is no cub temp storage, and the
// scan works on per-block partial sums.
struct GeomState {
    float* depths;            // [P]   view-space z
    float2* means2D;          // [P]   pixel centre
    float4* conic_opacity;    // [P]   conic.xyz, opacity
    float* cov3D;             // [P,6]
    float* rgb;               // [P,3] SH colours (only when shs given)
    uint8_t* clamped;         // [P,3]
    uint32_t* tiles_touched;  // [P]
    uint32_t* point_offsets;  // [P]   inclusive scan of tiles_touched
    int* radii;               // [P]   internal radii when the caller passes NULL
    uint32_t* block_sums;     // [ceil(P/256)+1] per-preprocess-block partial sums, then exclusive offsets
    uint32_t* counters;       // [8]   [0] = num_rendered
    float4* rec;              // [P,4] packed record the tile kernels gather: {x, y, depth, -} {conic.xyz, opacity} {r, g, b, -} {-}
};
struct ImgState {
    uint2* ranges;        // [T]
    float* final_T;       // [N]
    uint32_t* n_contrib;  // [N]
    uint32_t* median_pos; // [N] 1 + list position of the splat at which the pixel's T crossed 0.5 in the forward (0: it never did).
                          //     The reference's backward re-finds that splat from the T it reconstructs by division
                          //     (backward.cu:623-626, :854-857), which is exact only up to rounding: on a pixel whose T passes
                          //     within an ulp of 0.5 it picks a neighbour, none or two.  Recording the forward's own decision
                          //     makes the median-depth gradient land on exactly the splat whose depth the forward output.
};
struct BinState {
    uint64_t* keys_unsorted;  // [R]
    uint64_t* keys;           // [R]
    uint32_t* vals_unsorted;  // [R]
    uint32_t* vals;           // [R]
    uint32_t* hist;           // radix-sort per-block digit histograms
};

// Binning state resolved ON THE DEVICE from num_rendered (speculative forward, hsr_api.hip): the host enqueues the emit,
// per-tile sort and render kernels before it has read num_rendered back, so their array bases — which depend on it
// (hsr_carve_bin) — are derived by the kernels themselves from the device-side counter.  base == NULL: not used.
struct BinDevRef {
    char* base;               // the caller's binning buffer
    const uint32_t* R_dev;    // num_rendered, written by the scan
    size_t capacity;          // bytes usable from base
};
constexpr int HSR_SORT_TILE = 4096;   // pairs per radix-sort block (hsr_sort.hip)
__host__ __device__ inline uint32_t hsr_sort_hist_entries_inline(uint32_t R)
{
    const uint32_t nblocks = (R + HSR_SORT_TILE - 1) / HSR_SORT_TILE;
    return 256u * (nblocks > 0 ? nblocks : 1u) + 256u;
}

// ---- layouts of the three state buffers, stated once each (hsr_state.hip; the binning buffer's here, for the device): the byte
// offset of every array from a 256-aligned origin, every array 256-aligned, and `end`, the bytes used from that origin.  Integers
// only.  A carve aligns the real base up to 256 and adds the offsets; a size query is `end` plus 256 bytes for that alignment.
constexpr size_t hsr_align256(size_t v) { return (v + 255) & ~(size_t)255; }
struct GeomLayout { size_t depths, means2D, conic_opacity, cov3D, rgb, clamped, tiles_touched, point_offsets, radii, block_sums, counters, rec, end; };
struct ImgLayout { size_t ranges, final_T, n_contrib, median_pos, end; };
struct BinLayout { size_t keys_unsorted, keys, vals_unsorted, vals, hist, end; };
GeomLayout hsr_geom_layout(int P);
ImgLayout hsr_img_layout(int W, int H);
// the ONE rule of the binning buffer, counted from `origin`: 0 for offsets (a 256-aligned base), or an address as an integer, which
// is how the speculative kernels resolve their arrays from the device-side num_rendered (hsr_bin_resolve)
__host__ __device__ inline BinLayout hsr_bin_layout(size_t origin, uint32_t R)
{
    const size_t Rn = R > 0 ? R : 1;
    BinLayout l;
    size_t p = origin;
    p = (p + 255) & ~(size_t)255; l.keys_unsorted = p; p += 8 * Rn;
    p = (p + 255) & ~(size_t)255; l.keys = p; p += 8 * Rn;
    p = (p + 255) & ~(size_t)255; l.vals_unsorted = p; p += 4 * Rn;
    p = (p + 255) & ~(size_t)255; l.vals = p; p += 4 * Rn;
    p = (p + 255) & ~(size_t)255; l.hist = p; p += 4 * (size_t)hsr_sort_hist_entries_inline(R);
    l.end = p;
    return l;
}
// the arrays of R instances in the buffer at ref.base; false when it is too small for them
__host__ __device__ inline bool hsr_bin_resolve(const BinDevRef& ref, uint32_t R, BinState* out)
{
    const size_t base = reinterpret_cast<uintptr_t>(ref.base);
    const BinLayout l = hsr_bin_layout(base, R);
    out->keys_unsorted = reinterpret_cast<uint64_t*>(l.keys_unsorted);
    out->keys = reinterpret_cast<uint64_t*>(l.keys);
    out->vals_unsorted = reinterpret_cast<uint32_t*>(l.vals_unsorted);
    out->vals = reinterpret_cast<uint32_t*>(l.vals);
    out->hist = reinterpret_cast<uint32_t*>(l.hist);
    return l.end - base <= ref.capacity && R <= 0x7fffffffu;
}

void hsr_carve_geom(char* base, int P, GeomState* out);
void hsr_carve_img(char* base, int W, int H, ImgState* out);
void hsr_carve_bin(char* base, int R, BinState* out);   // R < 0 counts as 0

void hsr_set_error(const char* fmt, ...);

// Environment selectors the library reads, each once per process: HSR_BWD_IMPL=valu (the all-VALU backward) | legacy (accumulation
// mode 2) and HSR_SORT_IMPL=radix pick paths the default itself takes for some inputs and that give the same results
// (tests/test_gpu_golden_and_scale.py runs the parity cases under each); HSR_SEMANTIC_ALPHA=exact opts in to the semantic -> alpha term.

#define HSR_HIP_CHECK(expr)                                                                     \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess) {                                                                \
            hsr_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return HSR_ERR_HIP;                                                                 \
        }                                                                                       \
    } while (0)

// launch check: always catches launch-configuration errors; in debug mode also synchronises the
// stream so that a kernel fault is reported at its call site (reference CHECK_CUDA, auxiliary.h:166-173)
#define HSR_LAUNCH_CHECK(debug, stream)                            \
    do {                                                           \
        HSR_HIP_CHECK(hipGetLastError());                          \
        if (debug) HSR_HIP_CHECK(hipStreamSynchronize(stream));    \
    } while (0)

// ---- kernel launchers (one translation unit per stage) ----
struct PreprocessArgs {
    int P, D, M, W, H;
    const float* means3D;
    const float* scales;
    float scale_modifier;
    const float* rotations;
    const float* opacities;
    const float* shs;
    const float* cov3D_precomp;
    const float* colors_precomp;
    const float* viewmatrix;
    const float* projmatrix;
    const float* cam_pos;
    float tan_fovx, tan_fovy, focal_x, focal_y;
    int* radii;
    int prefiltered;
    int tiles_x, tiles_y;
};

int hsr_launch_mark_visible(int P, const float* means3D, const float* view, const float* proj, uint8_t* present,
                            hipStream_t stream);
int hsr_launch_preprocess(const PreprocessArgs& a, GeomState& g, hipStream_t stream);
int hsr_launch_scan_block_sums(int P, GeomState& g, hipStream_t stream);
int hsr_launch_duplicate(int P, const int* radii, int tiles_x, int tiles_y, GeomState& g, BinState& b, uint2* ranges,
                         hipStream_t stream);  // also zeroes ranges[0, tiles)
int hsr_launch_sort_pairs(BinState& b, int R, int end_bit, int T, uint2* ranges, hipStream_t stream);  // also fills ranges
struct HsrBinPlan { int nblk, per_block; };   // direct tile binning: workgroups and Gaussians per workgroup
bool hsr_bin_plan(int P, int T, size_t scratch_words, HsrBinPlan* plan);   // false = not applicable (radix path)
int hsr_launch_bin_count(const HsrBinPlan& plan, int P, const int* radii, int tiles_x, int tiles_y, GeomState& g, uint32_t* scratch,
                         uint2* ranges, hipStream_t stream, uint32_t* host_counter = nullptr, uint32_t host_seq = 0);
                         // per-tile counts; produces num_rendered (counters[0]; also {value, seq} into host-mapped memory)
// Order in which bin_scan_kernel sums the nblk rows of the count table (row b = workgroup b of bin_hist / bin_emit): the k-th row of
// "all rows with b mod 8 = 0 ascending, then b mod 8 = 1, ... then 7".  With q = nblk / 8 and r = nblk mod 8, class c has q + (c < r)
// rows; for nblk < 8 it is the identity.  Workgroups are dealt round-robin over the eight XCDs, so a class is what ONE L2 writes: a tile
// segment becomes eight sub-segments, each filled through one L2 (hsr_preprocess.hip, above bin_hist_kernel).  Speed only: any
// bijection gives the same sorted lists.
__host__ __device__ inline int hsr_bin_row_of(int k, int nblk)
{
    if (nblk < 8) return k;
    const int q = nblk >> 3, r = nblk & 7;
    const int big = r * (q + 1);   // the logical positions of the r classes that hold q + 1 rows
    if (k < big) {
        const int c = k / (q + 1);
        return 8 * (k - c * (q + 1)) + c;
    }
    const int m = k - big, c = m / q;
    return 8 * (m - c * q) + r + c;
}
// the row after row b in that order (b is not the last one): hsr_bin_row_of(k + 1) from hsr_bin_row_of(k) without the divisions
__host__ __device__ inline int hsr_bin_row_next(int b, int nblk) { return b + 8 < nblk ? b + 8 : (b & 7) + 1; }
// bin_scan_kernel, workgroup w of a grid of n -> its block of 16 tiles (64 bytes of every table row).  Two neighbouring blocks share
// each 128-byte line; inside a group of sixteen workgroups they go to w and w + 8, which one XCD runs.  The ragged last group keeps w.
__host__ __device__ inline int hsr_bin_scan_block_of(int w, int n)
{
    if ((w | 15) >= n) return w;
    return (w & ~15) + 2 * (w & 7) + ((w >> 3) & 1);
}
int hsr_launch_bin_emit(const HsrBinPlan& plan, int P, const int* radii, int tiles_x, int tiles_y, GeomState& g, const uint32_t* scratch,
                        uint2* ranges, uint64_t* comp, hipStream_t stream, const BinDevRef* ref = nullptr);
                        // tile ranges; (depth, index) composites into the tile segments
int hsr_launch_tile_sort(BinState& b, int T, int P, const uint2* ranges, hipStream_t stream, const BinDevRef* ref = nullptr,
                         int avg_per_tile_hint = 0);  // per-tile (depth, index) sort; hint: entries per tile of the previous frame
int hsr_sort_tile_passes(int end_bit);
bool hsr_sort_emit_into_sorted_buffers(int end_bit);
int hsr_launch_tile_ranges_only(int R, const uint64_t* keys, uint2* ranges, hipStream_t stream);

struct RenderFwdArgs {
    int W, H, K, semantic;
    const uint2* ranges;
    const uint32_t* point_list;
    uint32_t* masks;         // [R], parallel to point_list: the 16-bit sub-block mask of every list entry the forward stages (hsr_tile_common.h:
                             // subblock_mask), kept for the backward in BinState::vals_unsorted — free once the per-tile sort has run
    const float2* means2D;
    const float4* conic_opacity;
    const float* depths;
    const float* colors;     // [P,3]
    const float4* rec;       // packed per-Gaussian record (GeomState::rec): ONE 64-byte line instead of four arrays, or NULL
    const float* semantics;  // [P,K] or NULL
    float* final_T;
    uint32_t* n_contrib;
    uint32_t* median_pos;
    float* out_color;
    float* out_semantic;
    float* out_depth;
    float* out_median_depth;
    float* out_opacity;
    float* out_mask;  // non-semantic variant only
    BinDevRef bin;    // base != NULL: point_list is resolved on the device (speculative forward)
};
int hsr_launch_render_forward(const RenderFwdArgs& a, hipStream_t stream);

struct RenderBwdArgs {
    int W, H, K, semantic, P;
    const float* bg;  // device [3]
    const uint2* ranges;
    const uint32_t* point_list;
    const uint32_t* masks;   // [R] sub-block masks written by the forward's staging (RenderFwdArgs::masks)
    const float2* means2D;
    const float4* conic_opacity;
    const float* depths;
    const float* colors;
    const float4* rec;    // packed per-Gaussian record (GeomState::rec), or NULL
    const float* final_T;
    const uint32_t* n_contrib;
    const uint32_t* median_pos;
    const float* dL_dpix;
    const float* dL_dpix_sem;
    const float* dL_dpix_depth;
    const float* dL_dpix_median;
    const float* dL_dpix_opacity;
    float* dL_dmean2D;    // [P,3]
    float* dL_dconic;     // [P,4]
    float* dL_dopacity;   // [P]
    float* dL_dcolor;     // [P,3]
    float* dL_dsemantics; // [P,K]
    float* dL_ddepth;     // [P]
    float* grow;          // packed mode: [P][grow_stride] one gradient row per Gaussian (scratch), else NULL
    int grow_stride;
    int grow_layout;      // 0: classic packed row; 1: compact (hsr_tile_common.h, hsr_grow_col) — hsr_render_bwd_q.hip only
    const float* semantics = nullptr;   // [P,K] features: read by the exact semantic -> alpha passes only (hsr_launch_render_backward_qsema)
    int sem_c0 = 0;                      // ... first channel of the pass
};
// The matrix-core tile kernels address the packed rows with 32-bit element indices: P * stride must stay below 2^30.  The ONE
// statement of that limit: the plan (hsr_api.hip, plan_backward) decides with it, the launchers below check it.
inline bool hsr_rows_fit_32bit(int P, int stride) { return (size_t)P * (size_t)stride < ((size_t)1 << 30); }
// kernel: HSR_BWD_KERNEL_* of the call's hsr_backward_plan (include/hsr_rasterizer.h), whose layout and stride a.grow_* carry.
// The three specialised launchers refuse (HSR_ERR_INVALID_ARGUMENT, nothing launched) arguments their kernels cannot take.
int hsr_launch_render_backward(int kernel, const RenderBwdArgs& a, hipStream_t stream);
int hsr_launch_render_backward_q(const RenderBwdArgs& a, hipStream_t stream);     // K <= 27, packed mode: round 4, both per-pixel factors in LDS panels, moments per chunk
int hsr_launch_render_backward_qgeo(const RenderBwdArgs& a, hipStream_t stream);  // geometry gradients only, same scheme
int hsr_launch_render_backward_qsema(const RenderBwdArgs& a, hipStream_t stream); // packed rows: + the exact semantic -> alpha term into columns 0..5 (opt-in)
int hsr_launch_render_backward_subw(const RenderBwdArgs& a, hipStream_t stream);  // K > 27, packed mode: sub-block masks, channel passes

struct PreBwdArgs {
    int P, D, M;
    const float* means3D;
    const int* radii;
    const float* shs;
    const uint8_t* clamped;
    const float* scales;
    const float* rotations;
    float scale_modifier;
    const float* cov3Ds;
    const float* viewmatrix;
    const float* projmatrix;
    float focal_x, focal_y, tan_fovx, tan_fovy;
    const float* campos;
    const float* dL_dmean2D;
    const float* dL_dconic;
    float* dL_dmean3D;
    float* dL_dcolor;
    const float* dL_ddepth;
    float* dL_dcov3D;
    float* dL_dsh;
    float* dL_dscale;
    float* dL_drot;
    // packed mode: one atomically accumulated row per Gaussian (see hsr_grow_* in hsr_tile_common.h), unpacked into the out_* arrays
    int K;
    float *out_mean2D, *out_conic, *out_opacity, *out_color, *out_semantics, *out_depth;
    const float* grow;
    int grow_stride;
    int grow_layout;         // layout of the packed rows (RenderBwdArgs::grow_layout)
    int geo;                 // geometry-only rows (16 floats: columns 0..6, depth complete in column 6); out_color / out_opacity / out_semantics NULL
};
int hsr_launch_preprocess_backward(const PreBwdArgs& a, hipStream_t stream);
int hsr_launch_zero_visible_rows(int P, const int* radii, float* grow, int stride, hipStream_t stream);   // packed rows of visible Gaussians := 0

#ifndef HSR_OK
#define HSR_OK 0
#define HSR_ERR_INVALID_ARGUMENT (-1)
#define HSR_ERR_BUFFER_TOO_SMALL (-2)
#define HSR_ERR_HIP (-3)
#define HSR_ERR_NO_DEVICE (-4)
#endif

// ---- host helpers of the frame-sized units' entry points ----
// a frame the kernels cannot index: an empty side, or more pixels than a 32-bit int counts
inline bool hsr_bad_frame_size(int H, int W) { return H < 1 || W < 1 || (size_t)H * W > 0x7fffffffu; }

// the one scratch check: `who` is the entry point's name as it begins every message of that entry point
inline int hsr_check_scratch(const char* who, const char* scratch, size_t have, size_t need, unsigned align = 1)
{
    if (!scratch || have < need || (reinterpret_cast<uintptr_t>(scratch) & (align - 1)) != 0) {
        hsr_set_error("%s: scratch too small: %zu bytes needed, %zu given (or NULL, or not %u-byte aligned)", who, need, have, align);
        return HSR_ERR_BUFFER_TOO_SMALL;
    }
    return HSR_OK;
}
