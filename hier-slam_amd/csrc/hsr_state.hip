// hsr_state.hip — the layouts of the three caller-owned state buffers.  Host arithmetic only: no HIP runtime call, no launcher, so
// this unit links and is checked on its own.  Each layout is ONE function that counts byte offsets from a 256-aligned origin in
// size_t and forms no pointer (the binning buffer's is hsr_bin_layout in hsr_common.h, which the speculative kernels evaluate on the
// device).  The rest derives from it: a carve aligns the buffer's base up to 256 and adds the offsets, hsr_required_*_bytes is the
// layout's end plus the 256 bytes that alignment may cost, hsr_get_state_layout copies the offsets.
#include "../../include/hsr_rasterizer.h"
#include "hsr_tile_common.h"

namespace {

// the next array, `bytes` long: its 256-aligned offset; `end` moves behind it
size_t take(size_t& end, size_t bytes)
{
    const size_t at = hsr_align256(end);
    end = at + bytes;
    return at;
}

// the array at `offset` in the buffer at `base`, as an address computed in integers
template <typename T>
void place(T*& array, const char* base, size_t offset)
{
    array = reinterpret_cast<T*>(hsr_align256(reinterpret_cast<uintptr_t>(base)) + offset);
}

uint32_t instances(int R) { return (uint32_t)(R > 0 ? R : 0); }

}  // namespace

GeomLayout hsr_geom_layout(int P)
{
    const size_t Pn = (size_t)(P > 0 ? P : 1);
    GeomLayout l{};
    size_t& end = l.end;
    l.depths = take(end, Pn * sizeof(float));
    l.means2D = take(end, Pn * sizeof(float2));
    l.conic_opacity = take(end, Pn * sizeof(float4));
    l.cov3D = take(end, Pn * 6 * sizeof(float));
    l.rgb = take(end, Pn * 3 * sizeof(float));
    l.clamped = take(end, Pn * 3 * sizeof(uint8_t));
    l.tiles_touched = take(end, Pn * sizeof(uint32_t));
    l.point_offsets = take(end, Pn * sizeof(uint32_t));
    l.radii = take(end, Pn * sizeof(int));
    l.block_sums = take(end, ((Pn + 255) / 256 + 1) * sizeof(uint32_t));
    l.counters = take(end, 8 * sizeof(uint32_t));
    l.rec = take(end, Pn * 4 * sizeof(float4));
    return l;
}

ImgLayout hsr_img_layout(int W, int H)
{
    const size_t N = (size_t)W * H;
    const size_t T = (size_t)hsr_num_tiles(W, H);
    ImgLayout l{};
    size_t& end = l.end;
    l.ranges = take(end, T * sizeof(uint2));
    l.final_T = take(end, N * sizeof(float));
    l.n_contrib = take(end, N * sizeof(uint32_t));
    l.median_pos = take(end, N * sizeof(uint32_t));
    return l;
}

void hsr_carve_geom(char* base, int P, GeomState* out)
{
    const GeomLayout l = hsr_geom_layout(P);
    place(out->depths, base, l.depths); place(out->means2D, base, l.means2D); place(out->conic_opacity, base, l.conic_opacity);
    place(out->cov3D, base, l.cov3D); place(out->rgb, base, l.rgb); place(out->clamped, base, l.clamped);
    place(out->tiles_touched, base, l.tiles_touched); place(out->point_offsets, base, l.point_offsets); place(out->radii, base, l.radii);
    place(out->block_sums, base, l.block_sums); place(out->counters, base, l.counters); place(out->rec, base, l.rec);
}

void hsr_carve_img(char* base, int W, int H, ImgState* out)
{
    const ImgLayout l = hsr_img_layout(W, H);
    place(out->ranges, base, l.ranges); place(out->final_T, base, l.final_T);
    place(out->n_contrib, base, l.n_contrib); place(out->median_pos, base, l.median_pos);
}

void hsr_carve_bin(char* base, int R, BinState* out)
{
    const BinLayout l = hsr_bin_layout(0, instances(R));
    place(out->keys_unsorted, base, l.keys_unsorted); place(out->keys, base, l.keys);
    place(out->vals_unsorted, base, l.vals_unsorted); place(out->vals, base, l.vals); place(out->hist, base, l.hist);
}

extern "C" {

size_t hsr_required_geometry_bytes(int P) { return hsr_geom_layout(P).end + 256; }
size_t hsr_required_image_bytes(int width, int height) { return hsr_img_layout(width, height).end + 256; }
size_t hsr_required_binning_bytes(int num_rendered) { return hsr_bin_layout(0, instances(num_rendered)).end + 256; }

int hsr_get_state_layout(int P, int width, int height, int num_rendered, hsr_state_layout* out)
{
    if (!out) return HSR_ERR_INVALID_ARGUMENT;
    const GeomLayout g = hsr_geom_layout(P);
    const ImgLayout im = hsr_img_layout(width, height);
    const BinLayout b = hsr_bin_layout(0, instances(num_rendered));
    out->geom_depths = g.depths; out->geom_means2D = g.means2D; out->geom_conic_opacity = g.conic_opacity;
    out->geom_cov3D = g.cov3D; out->geom_rgb = g.rgb; out->geom_clamped = g.clamped;
    out->geom_tiles_touched = g.tiles_touched; out->geom_point_offsets = g.point_offsets; out->geom_radii = g.radii;
    out->bin_keys_unsorted = b.keys_unsorted; out->bin_keys = b.keys; out->bin_vals_unsorted = b.vals_unsorted;
    out->bin_vals = b.vals;
    out->img_ranges = im.ranges; out->img_final_T = im.final_T; out->img_n_contrib = im.n_contrib;
    out->img_median_pos = im.median_pos;
    return HSR_OK;
}

}  // extern "C"
