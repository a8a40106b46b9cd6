// hostcheck.hip — a stand-alone check of the rasterizer's host layer (csrc/hsr_api.hip + csrc/hsr_state.hip) under the host
// sanitizers: `make -C hier-slam_amd/csrc hostcheck` builds those units with ASan + UBSan, links them with this file and runs it.
// It has its own main and its own definitions of the 15 launcher symbols the API unit imports, each of which only counts its
// calls.  Every call made here returns before the HIP runtime is touched, so it needs no GPU and must not be run on one's machine;
// that no stub was ever called is the proof that a refused call has enqueued nothing.  Output: one line per section, then
// "hostcheck: OK" (exit 0) or the failed checks (exit 1).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/hsr_rasterizer.h"
#include "../hier-slam_amd/csrc/hsr_tile_common.h"

static int g_stub_calls = 0, g_failed = 0, g_checks = 0;

#define CHECK(cond)                                                         \
    do {                                                                    \
        ++g_checks;                                                         \
        if (!(cond)) {                                                      \
            ++g_failed;                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
        }                                                                   \
    } while (0)

// ---- the launchers: counted, never expected ----
int hsr_launch_mark_visible(int, const float*, const float*, const float*, uint8_t*, hipStream_t) { return ++g_stub_calls; }
int hsr_launch_preprocess(const PreprocessArgs&, GeomState&, hipStream_t) { return ++g_stub_calls; }
int hsr_launch_scan_block_sums(int, GeomState&, hipStream_t) { return ++g_stub_calls; }
int hsr_launch_duplicate(int, const int*, int, int, GeomState&, BinState&, uint2*, hipStream_t) { return ++g_stub_calls; }
int hsr_launch_sort_pairs(BinState&, int, int, int, uint2*, hipStream_t) { return ++g_stub_calls; }
bool hsr_bin_plan(int, int, size_t, HsrBinPlan*) { return ++g_stub_calls != 0; }
int hsr_launch_bin_count(const HsrBinPlan&, int, const int*, int, int, GeomState&, uint32_t*, uint2*, hipStream_t, uint32_t*, uint32_t)
{
    return ++g_stub_calls;
}
int hsr_launch_bin_emit(const HsrBinPlan&, int, const int*, int, int, GeomState&, const uint32_t*, uint2*, uint64_t*, hipStream_t,
                        const BinDevRef*)
{
    return ++g_stub_calls;
}
int hsr_launch_tile_sort(BinState&, int, int, const uint2*, hipStream_t, const BinDevRef*, int) { return ++g_stub_calls; }
bool hsr_sort_emit_into_sorted_buffers(int) { return ++g_stub_calls != 0; }
int hsr_launch_render_forward(const RenderFwdArgs&, hipStream_t) { return ++g_stub_calls; }
int hsr_launch_render_backward(int, const RenderBwdArgs&, hipStream_t) { return ++g_stub_calls; }
int hsr_launch_render_backward_qsema(const RenderBwdArgs&, hipStream_t) { return ++g_stub_calls; }
int hsr_launch_preprocess_backward(const PreBwdArgs&, hipStream_t) { return ++g_stub_calls; }
int hsr_launch_zero_visible_rows(int, const int*, float*, int, hipStream_t) { return ++g_stub_calls; }

static const int GRID_P[] = {0, 1, 255, 256, 257, 1000, 500000};
static const int GRID_WH[][2] = {{1, 1}, {16, 16}, {17, 31}, {64, 48}, {1200, 680}, {1920, 1080}};
static const int GRID_R[] = {0, 1, 4095, 4096, 4097, 5000, 3000000, 2147483647};

// ---- 1. the size and layout queries over the grid of tests/golden/state_layout.json ----
static void check_grid()
{
    for (int P : GRID_P)
        for (const auto& wh : GRID_WH)
            for (int R : GRID_R) {
                hsr_state_layout l;
                CHECK(hsr_get_state_layout(P, wh[0], wh[1], R, &l) == HSR_OK);
                CHECK(l.geom_depths == 0 && l.img_ranges == 0 && l.bin_keys_unsorted == 0);
                CHECK(l.geom_radii % 256 == 0 && l.geom_radii < hsr_required_geometry_bytes(P));
                CHECK(l.img_median_pos % 256 == 0 && l.img_median_pos < hsr_required_image_bytes(wh[0], wh[1]));
                CHECK(l.bin_vals % 256 == 0 && l.bin_vals < hsr_required_binning_bytes(R));
            }
    CHECK(hsr_get_state_layout(1, 1, 1, 1, nullptr) == HSR_ERR_INVALID_ARGUMENT);
    CHECK(hsr_required_geometry_bytes(1000) == 144640 && hsr_required_image_bytes(64, 48) == 37376);
    CHECK(hsr_required_binning_bytes(5000) == 124160);
    hsr_state_layout l;
    hsr_get_state_layout(1000, 64, 48, 5000, &l);
    CHECK(l.img_final_T == 256 && l.bin_vals == 100608);
    printf("grid: %zu layouts queried\n", sizeof(GRID_P) / sizeof(int) * (sizeof(GRID_WH) / sizeof(GRID_WH[0])) * (sizeof(GRID_R) / sizeof(int)));
}

// ---- 2. the backward's plan ----
static void check_plans()
{
    const int Ks[] = {0, 16, 26, 27, 74}, Ps[] = {0, 1, 1000, 500000, 40000000};
    for (int K : Ks)
        for (int P : Ps)
            for (int geo = 0; geo < 2; ++geo) {
                hsr_backward_plan as_planned, none;
                CHECK(hsr_plan_backward(P, K, geo, HSR_SCRATCH_AS_PLANNED, &as_planned) == HSR_OK);
                CHECK(hsr_plan_backward(P, K, geo, 0, &none) == HSR_OK);
                CHECK(none.accumulation == 2 && none.kernel == HSR_BWD_KERNEL_VALU && none.scratch_bytes == 0);
                CHECK(as_planned.accumulation == (P > 0 ? 0 : 2));
                if (P > 0) CHECK(as_planned.scratch_bytes == hsr_backward_scratch_bytes(P, K, 0) && as_planned.row_stride % 16 == 0);
            }
    hsr_backward_plan p;
    CHECK(hsr_plan_backward(-1, 0, 0, 0, &p) == HSR_ERR_INVALID_ARGUMENT && strstr(hsr_last_error(), "hsr_plan_backward"));
    CHECK(hsr_plan_backward(1, 0, 0, 0, nullptr) == HSR_ERR_INVALID_ARGUMENT);
    printf("plans: K in {0, 16, 26, 27, 74} at five P\n");
}

// ---- 3. carves of real, deliberately misaligned host blocks ----
struct Array {
    const char* name;
    const void* at;
    size_t bytes;
    size_t offset;   // as hsr_get_state_layout reports it; NOT_REPORTED: the public layout does not carry this array
};
static const size_t NOT_REPORTED = ~(size_t)0;

static void check_arrays(const char* what, const char* base, size_t required, const Array* a, int n)
{
    const uintptr_t lo = reinterpret_cast<uintptr_t>(base), origin = (lo + 255) & ~(uintptr_t)255;
    CHECK(lo % 256 != 0);
    uintptr_t prev_end = lo;
    for (int i = 0; i < n; ++i) {
        const uintptr_t p = reinterpret_cast<uintptr_t>(a[i].at);
        const bool ok = p % 256 == 0 && p >= prev_end && p + a[i].bytes <= lo + required &&
                        (a[i].offset == NOT_REPORTED || p == origin + a[i].offset);
        CHECK(ok);
        if (!ok) printf("    %s.%s: at base + %zu, %zu bytes, previous array ends at base + %zu, buffer of %zu bytes\n", what, a[i].name,
                        (size_t)(p - lo), a[i].bytes, (size_t)(prev_end - lo), required);
        prev_end = p + a[i].bytes;
    }
}

static void check_carves()
{
    int carved = 0;
    for (int P : {0, 1, 257, 1000})
        for (const auto& wh : {GRID_WH[0], GRID_WH[2], GRID_WH[3]})
            for (int R : {0, 1, 4097, 5000}) {
                const int W = wh[0], H = wh[1];
                hsr_state_layout l;
                hsr_get_state_layout(P, W, H, R, &l);
                const size_t Pn = P > 0 ? P : 1, N = (size_t)W * H, T = (size_t)hsr_num_tiles(W, H), Rn = R > 0 ? R : 1;
                const size_t gb = hsr_required_geometry_bytes(P), ib = hsr_required_image_bytes(W, H), bb = hsr_required_binning_bytes(R);
                char* blocks[3] = {(char*)malloc(gb + 16), (char*)malloc(ib + 16), (char*)malloc(bb + 16)};
                GeomState g;
                ImgState im;
                BinState b;
                hsr_carve_geom(blocks[0] + 8, P, &g);
                hsr_carve_img(blocks[1] + 8, W, H, &im);
                hsr_carve_bin(blocks[2] + 8, R, &b);
                const Array ga[] = {{"depths", g.depths, 4 * Pn, l.geom_depths}, {"means2D", g.means2D, 8 * Pn, l.geom_means2D},
                                    {"conic_opacity", g.conic_opacity, 16 * Pn, l.geom_conic_opacity},
                                    {"cov3D", g.cov3D, 24 * Pn, l.geom_cov3D}, {"rgb", g.rgb, 12 * Pn, l.geom_rgb},
                                    {"clamped", g.clamped, 3 * Pn, l.geom_clamped},
                                    {"tiles_touched", g.tiles_touched, 4 * Pn, l.geom_tiles_touched},
                                    {"point_offsets", g.point_offsets, 4 * Pn, l.geom_point_offsets},
                                    {"radii", g.radii, 4 * Pn, l.geom_radii},
                                    {"block_sums", g.block_sums, 4 * ((Pn + 255) / 256 + 1), NOT_REPORTED},
                                    {"counters", g.counters, 32, NOT_REPORTED}, {"rec", g.rec, 64 * Pn, NOT_REPORTED}};
                const Array ia[] = {{"ranges", im.ranges, 8 * T, l.img_ranges}, {"final_T", im.final_T, 4 * N, l.img_final_T},
                                    {"n_contrib", im.n_contrib, 4 * N, l.img_n_contrib},
                                    {"median_pos", im.median_pos, 4 * N, l.img_median_pos}};
                const Array ba[] = {{"keys_unsorted", b.keys_unsorted, 8 * Rn, l.bin_keys_unsorted}, {"keys", b.keys, 8 * Rn, l.bin_keys},
                                    {"vals_unsorted", b.vals_unsorted, 4 * Rn, l.bin_vals_unsorted}, {"vals", b.vals, 4 * Rn, l.bin_vals},
                                    {"hist", b.hist, 4 * (size_t)hsr_sort_hist_entries_inline((uint32_t)R), NOT_REPORTED}};
                check_arrays("geometry", blocks[0] + 8, gb, ga, 12);
                check_arrays("image", blocks[1] + 8, ib, ia, 4);
                check_arrays("binning", blocks[2] + 8, bb, ba, 5);
                // the device's rule finds the same arrays in the same buffer, and just fits a buffer of the required size
                BinState r;
                CHECK(hsr_bin_resolve(BinDevRef{blocks[2] + 8, nullptr, bb}, (uint32_t)R, &r));
                CHECK(r.keys_unsorted == b.keys_unsorted && r.keys == b.keys && r.vals_unsorted == b.vals_unsorted && r.vals == b.vals &&
                      r.hist == b.hist);
                CHECK(!hsr_bin_resolve(BinDevRef{blocks[2] + 8, nullptr, bb - 256}, (uint32_t)R, &r));
                for (char* blk : blocks) free(blk);
                ++carved;
            }
    printf("carves: %d x 3 misaligned buffers\n", carved);
}

// ---- 4. every refusal that depends on the arguments alone: its code, its message, and nothing enqueued ----
static float g_dummy[64];   // stands for device memory: the refusals compare pointers with NULL and never follow them
static float* const D = g_dummy;
static char* const DC = reinterpret_cast<char*>(g_dummy);

struct Fwd {   // the arguments of hsr_forward[_semantic]; plausible by default
    int P = 10, Dg = 0, M = 0, K = 4, W = 32, H = 16;
    const float *means3D = D, *shs = nullptr, *colors = D, *semantics = D, *opacities = D, *scales = D, *rotations = D, *cov3D = nullptr,
                *view = D, *proj = D, *cam_pos = D;
    float *out_color = D, *out_semantic = D, *out_depth = D, *out_median = D, *out_opacity = D, *out_mask = D;
    int plain() const
    {
        return hsr_forward(nullptr, nullptr, nullptr, P, Dg, M, D, W, H, means3D, shs, colors, opacities, scales, 1.f, rotations, cov3D, view,
                           proj, cam_pos, 1.f, 1.f, 0, out_color, out_depth, out_median, out_opacity, out_mask, nullptr, 0, nullptr);
    }
    int sem() const
    {
        return hsr_forward_semantic(nullptr, nullptr, nullptr, P, Dg, M, K, D, W, H, means3D, shs, colors, semantics, opacities, scales, 1.f,
                                    rotations, cov3D, view, proj, cam_pos, 1.f, 1.f, 0, out_color, out_semantic, out_depth, out_median,
                                    out_opacity, nullptr, 0, nullptr);
    }
};

struct Bwd {   // the arguments of hsr_backward[_semantic]
    int P = 10, Dg = 0, M = 0, K = 4, R = 100, W = 32, H = 16;
    const float *bg = D, *shs = nullptr, *colors = D, *semantics = D, *scales = D, *rotations = D, *campos = D;
    const char *geom = DC, *binning = DC, *img = DC;
    const float *dL_dpix = D, *dL_dpix_sem = D, *dL_dpix_depth = D;
    float *dL_dmean2D = D, *dL_dconic = D, *dL_dopacity = D, *dL_dcolor = D, *dL_dsemantics = D, *dL_ddepth = D, *dL_dmean3D = D, *dL_dsh = D;
    char* scratch = nullptr;
    size_t scratch_bytes = 0;
    int plain() const
    {
        return hsr_backward(P, Dg, M, R, bg, W, H, D, shs, colors, scales, 1.f, rotations, nullptr, D, D, campos, 1.f, 1.f, nullptr, geom,
                            binning, img, dL_dpix, dL_dpix_depth, D, D, dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_ddepth, dL_dmean3D,
                            nullptr, dL_dsh, D, D, scratch, scratch_bytes, 0, nullptr);
    }
    int sem() const
    {
        return hsr_backward_semantic(P, Dg, M, K, R, bg, W, H, D, shs, colors, semantics, scales, 1.f, rotations, nullptr, D, D, campos, 1.f,
                                     1.f, nullptr, geom, binning, img, dL_dpix, dL_dpix_sem, dL_dpix_depth, D, D, dL_dmean2D, dL_dconic,
                                     dL_dopacity, dL_dcolor, dL_dsemantics, dL_ddepth, dL_dmean3D, nullptr, dL_dsh, D, D, scratch,
                                     scratch_bytes, 0, nullptr);
    }
};

#define REFUSED(call, message)                                                                                      \
    do {                                                                                                            \
        const int rc__ = (call);                                                                                    \
        ++g_checks;                                                                                                 \
        if (rc__ != HSR_ERR_INVALID_ARGUMENT || !strstr(hsr_last_error(), message)) {                               \
            ++g_failed;                                                                                             \
            printf("FAILED %s:%d: %s returned %d \"%s\", expected -1 \"%s\"\n", __FILE__, __LINE__, #call, rc__,    \
                   hsr_last_error(), message);                                                                      \
        }                                                                                                           \
        ++g_refusals;                                                                                               \
    } while (0)
static int g_refusals = 0;

static void check_refusals()
{
    // a call with nothing to refuse gets as far as its first acquire, whose NULL descriptor it reports
    REFUSED(Fwd().plain(), "geometry buffer descriptor is NULL");
    REFUSED(Fwd().sem(), "geometry buffer descriptor is NULL");
    Fwd f;
    f = Fwd(); f.P = -1; REFUSED(f.plain(), "invalid sizes P=-1 W=32 H=16"); REFUSED(f.sem(), "invalid sizes");
    f = Fwd(); f.W = 0; REFUSED(f.plain(), "invalid sizes"); f = Fwd(); f.H = -3; REFUSED(f.sem(), "invalid sizes");
    f = Fwd(); f.out_color = nullptr; REFUSED(f.plain(), "an output image pointer is NULL");
    f = Fwd(); f.out_opacity = nullptr; REFUSED(f.sem(), "an output image pointer is NULL");
    f = Fwd(); f.out_semantic = nullptr; REFUSED(f.sem(), "an output image pointer is NULL");
    f = Fwd(); f.K = -1; REFUSED(f.sem(), "K must be >= 0");
    f = Fwd(); f.means3D = nullptr; REFUSED(f.plain(), "means3D, opacities, viewmatrix and projmatrix are required");
    f = Fwd(); f.proj = nullptr; REFUSED(f.sem(), "means3D, opacities, viewmatrix and projmatrix are required");
    f = Fwd(); f.colors = nullptr; REFUSED(f.plain(), "provide colors_precomp, or shs with M > 0 and cam_pos");
    f = Fwd(); f.colors = nullptr; f.shs = D; f.M = 0; REFUSED(f.sem(), "provide colors_precomp, or shs with M > 0 and cam_pos");
    f = Fwd(); f.rotations = nullptr; REFUSED(f.plain(), "provide cov3D_precomp, or scales and rotations");
    f = Fwd(); f.semantics = nullptr; REFUSED(f.sem(), "semantics_precomp is NULL but K=4");
    f = Fwd(); f.colors = nullptr; f.shs = D; f.Dg = 2; f.M = 4; REFUSED(f.plain(), "SH degree 2 needs M >= 9 coefficients (got 4)");
    f = Fwd(); f.colors = nullptr; f.shs = D; f.Dg = 4; f.M = 25; REFUSED(f.sem(), "SH degree 4 needs");
    f = Fwd(); f.out_mask = nullptr; REFUSED(f.plain(), "out_mask is NULL");   // used to come after preprocess and the count

    Bwd b;
    CHECK(hsr_set_backward_mode(0) == HSR_OK && hsr_set_semantic_alpha_mode(0) == HSR_OK);
    b = Bwd(); b.P = 0; CHECK(b.plain() == HSR_OK && b.sem() == HSR_OK);   // nothing to do, nothing enqueued
    b = Bwd(); b.R = -1; REFUSED(b.plain(), "invalid sizes P=10 W=32 H=16 R=-1"); b = Bwd(); b.W = 0; REFUSED(b.sem(), "invalid sizes");
    b = Bwd(); b.geom = nullptr; REFUSED(b.plain(), "state buffers from the forward call are required");
    b = Bwd(); b.binning = nullptr; REFUSED(b.sem(), "state buffers from the forward call are required");
    b = Bwd(); b.dL_dpix = nullptr; REFUSED(b.plain(), "an upstream-gradient pointer is NULL");
    b = Bwd(); b.dL_dpix_sem = nullptr; REFUSED(b.sem(), "an upstream-gradient pointer is NULL");
    b = Bwd(); b.dL_dsemantics = nullptr; REFUSED(b.sem(), "an upstream-gradient pointer is NULL");
    b = Bwd(); b.dL_dmean2D = nullptr; REFUSED(b.plain(), "a gradient output pointer is NULL");
    b = Bwd(); b.dL_dcolor = nullptr; REFUSED(b.sem(), "a gradient output pointer is NULL");
    b = Bwd(); b.rotations = nullptr; REFUSED(b.plain(), "scales given without rotations");
    b = Bwd(); b.bg = nullptr; REFUSED(b.sem(), "background is NULL");
    // checks on the plan (pure arithmetic): without scratch the call is a legacy one
    b = Bwd(); b.dL_dcolor = b.dL_dopacity = b.dL_dsemantics = nullptr;
    REFUSED(b.plain(), "may only all be NULL (geometry-only gradients) in the packed accumulation mode");
    REFUSED(b.sem(), "may only all be NULL (geometry-only gradients) in the packed accumulation mode");
    b = Bwd(); b.dL_dconic = nullptr; REFUSED(b.plain(), "dL_dconic and dL_ddepth may only be NULL when a scratch buffer");
    b = Bwd(); b.dL_ddepth = nullptr; REFUSED(b.sem(), "dL_dconic and dL_ddepth may only be NULL when a scratch buffer");
    CHECK(hsr_set_semantic_alpha_mode(1) == HSR_OK && hsr_get_semantic_alpha_mode() == 1);
    REFUSED(Bwd().sem(), "the exact semantic -> alpha mode needs the packed accumulation mode");
    b = Bwd(); b.scratch = DC; b.scratch_bytes = hsr_backward_scratch_bytes(b.P, b.K, b.R); b.semantics = nullptr;
    REFUSED(b.sem(), "the exact semantic -> alpha mode reads semantics_precomp, which is NULL");
    CHECK(hsr_set_semantic_alpha_mode(0) == HSR_OK);
    b = Bwd(); b.colors = nullptr; b.shs = D; b.M = 1; b.dL_dsh = nullptr;
    REFUSED(b.plain(), "shs given without dL_dsh / campos");                   // used to come after the tile backward
    b.dL_dsh = D; b.campos = nullptr; REFUSED(b.sem(), "shs given without dL_dsh / campos");
    b.scratch = DC; b.scratch_bytes = hsr_backward_scratch_bytes(b.P, b.K, b.R);
    REFUSED(b.plain(), "shs given without dL_dsh / campos");                   // the packed mode as well

    hsr_ticket tk;
    memset(&tk, 0, sizeof(tk));
    REFUSED(hsr_forward_end(nullptr, 1, nullptr), "hsr_forward_end: the ticket does not belong to a forward call that ran ahead");
    REFUSED(hsr_forward_end(&tk, 0, nullptr), "hsr_forward_end: the ticket does not belong");
    tk.seq = 7; REFUSED(hsr_forward_end(&tk, 1, nullptr), "hsr_forward_end: the ticket does not belong");
    REFUSED(hsr_mark_visible(-1, D, D, D, reinterpret_cast<uint8_t*>(DC), nullptr), "hsr_mark_visible: invalid arguments");
    REFUSED(hsr_mark_visible(5, nullptr, D, D, reinterpret_cast<uint8_t*>(DC), nullptr), "hsr_mark_visible: invalid arguments");
    REFUSED(hsr_mark_visible(5, D, D, D, nullptr, nullptr), "hsr_mark_visible: invalid arguments");
    REFUSED(hsr_set_backward_mode(3), "backward mode must be 0 (packed), 1 (rows) or 2 (legacy)");
    REFUSED(hsr_set_backward_mode(-1), "backward mode must be");
    REFUSED(hsr_set_backward_mode(1), "the per-instance rows mode was an experiment");
    REFUSED(hsr_set_semantic_alpha_mode(2), "semantic alpha mode must be 0");
    CHECK(hsr_get_backward_mode() == 0 && hsr_get_semantic_alpha_mode() == 0);
    printf("refusals: %d calls\n", g_refusals);
}

int main()
{
    check_grid();
    check_plans();
    check_carves();
    check_refusals();
    CHECK(g_stub_calls == 0);
    printf("launcher stubs called: %d\n", g_stub_calls);
    if (g_failed) {
        printf("hostcheck: %d of %d checks FAILED\n", g_failed, g_checks);
        return 1;
    }
    printf("hostcheck: OK (%d checks)\n", g_checks);
    return 0;
}
