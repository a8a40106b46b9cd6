"""CPU suite: the first-frame-style scenes of tests/scenes.py (sensor_grid, TIE_CASES) stay in the regime they were chosen for.

Every other scene of the suite comes from hsr_utils.synthetic.make_scene: continuous random depths seen through a tilted camera, so
two splats of a tile almost never share a depth (0-156 equal neighbours in lists of 7 200-240 000 entries) and the index half of the
sort's composite key (depth bits << 32) | index decides nothing.  A map built from a quantised sensor depth image and viewed from the
identity pose is the opposite: nearly every neighbour in a tile's list has the same depth bits, and the blend order among them — alpha
blending does not commute — is the ascending Gaussian index of the reference's stable sort (rasterizer_impl.cu:307-312) and nothing else.

Here, on the oracle alone: the share of equal neighbours, the size class of the per-tile sort each scene reaches, the oracle's own rule
among ties, the caps tests/test_gpu_parity.py::_compare applies to the oracle's threshold-tie bookkeeping, and — for the cases whose
floats the GPU suite compares — that the fp32 oracle agrees with its truth build, so that a float mismatch on the device is the
device's.  tests/test_gpu_depth_ties.py then holds the HIP path to these lists bit for bit.

Measured on the oracle (entries per tile; equal adjacent keys of all adjacent pairs; tie-risk pixels / cap):

    first_frame            P  6 144   R    11 896   361-578     11 075 / 11 895 = 93.1 %        2 / 30    floats agree with the truth
    first_frame_shuffled   P  6 144   R    11 896   361-578     93.1 %                          3 / 30    floats agree
    wide                   P  3 072   R    12 036   634-1502    11 950 / 12 035 = 99.3 %        3 / 15    floats agree
    wide_shuffled          P  3 072   R    12 036   634-1502    99.3 %                          1 / 15    floats agree
    deep                   P  3 072   R    22 758   1308-2683   22 710 / 22 757 = 99.8 %        3 / 15    floats agree   (4 of 12 tiles > 2048)
    deep_65537             P 69 888   R 1 019 039   1785-5026   1 018 342 / 1 019 038 = 99.9 %  207 / 349 integers only  (269 tiles > 2048)
    deep_65537_two_exponents    as deep_65537, the ramp from 1 m: 212 / 349 tie-risk pixels; 73 of its 269 tiles > 2048 hold depths on both sides of 2.0
    small                  P    384   R       640   81-132      604 / 639 = 94.5 %              0 / 8     floats agree
    one_tile_256           P    256   R       256   256         254 / 255 = 99.6 %              0 / 8     floats agree
    duplicates             P  7 144   R    13 342   361-789     12 521 / 13 341 = 93.9 %        4 / 30    floats agree   (duplicate_first = 1000)

The oracle takes 1.3 s on deep_65537 and at most half a second on any other case."""
import numpy as np
import pytest

import scenes
from harness import assert_close, run_oracle

MIN_TIE_SHARE = 0.9


def _ranges(st):
    return st.field("ranges").reshape(-1, 2).astype(np.int64)


def _lists(st):
    rng = _ranges(st)
    return st.field("keys"), st.field("vals"), rng[:, 1] - rng[:, 0]


@pytest.mark.parametrize("name", list(scenes.TIE_CASES))
def test_scene_stays_in_its_regime_and_the_oracle_orders_ties_by_index(name):
    kw, lo_class, hi_class, floats = scenes.TIE_CASES[name]
    cam, sc, up = scenes.sensor_grid(**kw)
    W, H = kw["W"], kw["H"]
    out, gr, st = run_oracle(cam, sc, up, semantic=True)
    try:
        keys, vals, n = _lists(st)
        share = scenes.tie_share(keys)
        tie_px = int(st.field("tie_pixels").astype(bool).sum())
        print("%s: P %d R %d, entries per tile %d-%d (%d tiles > 2048), equal adjacent keys %.4f, tie-risk pixels %d (cap %d)"
              % (name, sc["means3D"].shape[0], keys.size, n.min(), n.max(), int((n > 2048).sum()), share, tie_px, max(8, W * H // 200)))
        assert keys.size == out["num_rendered"] == int(n.sum())
        assert share >= MIN_TIE_SHARE, share
        assert lo_class[0] <= n.min() <= lo_class[1], (int(n.min()), lo_class)
        assert hi_class[0] <= n.max() <= hi_class[1], (int(n.max()), hi_class)
        assert bool((keys[1:] >= keys[:-1]).all())
        scenes.assert_ties_in_index_order(keys, vals)
        if name == "deep_65537_two_exponents":
            # the block radix sort's last pass (the most significant depth byte) has something to move in a tile that takes seven passes
            top = (keys & np.uint64(0xFFFFFFFF)) >> np.uint64(24)
            mixed = sum(int(top[a:b].min() != top[a:b].max()) for a, b in _ranges(st)[n > 2048])
            print("%s: %d of %d tiles > 2048 entries hold two most significant depth bytes" % (name, mixed, int((n > 2048).sum())))
            assert mixed > 0
        # the caps _compare holds the oracle's threshold-tie bookkeeping to
        assert tie_px <= max(8, W * H // 200), tie_px
        assert st.bounds_info["overflow_pixels"] == 0, st.bounds_info
        if not floats:
            return
        out_t, gr_t, st_t = run_oracle(cam, sc, up, semantic=True, precision="f64", bounds=False)
        try:
            assert np.array_equal(st_t.field("keys"), keys) and np.array_equal(st_t.field("vals"), vals)
            for nme in ("color", "depth", "opacity", "semantic"):
                assert_close(nme, out[nme], out_t[nme])
            for nme in gr:
                assert_close("grad " + nme, gr[nme], gr_t[nme], rtol=1e-4, atol=1e-4)
        finally:
            st_t.free()
    finally:
        st.free()


def test_block_radix_cases_reach_the_pass_counts_they_are_named_for():
    """The block radix sort of hsr_sort.hip runs ceil(ceil(log2 P) / 8) index passes before its four depth passes.  `deep` has two (six in
    all: the segment ends where it began); `deep_65537` needs P > 65 536 for three (seven: the copy home at the end) and tiles beyond
    2 048 entries to get there at all.  Leaving the copy out shows only where the seventh pass moves something: `deep_65537_two_exponents`."""
    def index_passes(P):
        bits = 0
        while (1 << bits) < max(P, 1):
            bits += 1
        return (bits + 7) // 8
    for name, passes in (("deep", 2), ("deep_65537", 3), ("deep_65537_two_exponents", 3)):
        kw = scenes.TIE_CASES[name][0]
        P = len(range(0, kw["W"], kw.get("stride", 1))) * len(range(0, kw["H"], kw.get("stride", 1))) + kw.get("duplicate_first", 0)
        assert index_passes(P) == passes, (name, P)
    assert (index_passes(69888) + 4) % 2 == 1 and (index_passes(3072) + 4) % 2 == 0


def test_shuffle_and_duplicates_change_the_index_order_only():
    """shuffle: the same splats under other indices — the same sorted keys, and the sorted values are the unshuffled ones renamed.
    duplicate_first: a copy follows its original in every list they share, with nothing but entries of the same key and of indices in
    between between them."""
    import oracle_lib as O

    def lists(kw):
        cam, sc, up = scenes.sensor_grid(**kw)
        out, st = O.forward(cam, sc["means3D"], sc["opacities"], colors_precomp=sc["colors_precomp"],
                            semantics_precomp=sc["semantics_precomp"], scales=sc["scales"], rotations=sc["rotations"])
        k, v = st.field("keys").copy(), st.field("vals").astype(np.int64)
        st.free()
        return sc, k, v
    kw = scenes.TIE_CASES["first_frame"][0]
    sc0, k0, v0 = lists(kw)
    sc1, k1, v1 = lists(dict(kw, shuffle=True))
    assert np.array_equal(k0, k1) and not np.array_equal(v0, v1)
    # shuffled Gaussian j is raster Gaussian perm[j] (sensor_grid's permutation): under every key the same set of splats
    import torch
    perm = torch.randperm(sc0["means3D"].shape[0], generator=torch.Generator(device="cpu").manual_seed(3)).numpy()
    assert np.array_equal(sc1["means3D"].numpy(), sc0["means3D"].numpy()[perm])
    renamed = perm[v1]
    assert np.array_equal(v0, renamed[np.lexsort((renamed, k1))])
    # duplicates
    n = 1000
    sc2, k2, v2 = lists(dict(kw, duplicate_first=n))
    P = sc0["means3D"].shape[0]
    assert sc2["means3D"].shape[0] == P + n
    copies = np.flatnonzero(v2 >= P)
    assert copies.size > 0 and bool((k2[copies] == k2[copies - 1]).all())
    originals = v2[copies] - P
    # between an original and its copy only entries of the same key and of indices in between
    for pos, orig in zip(copies[:200], originals[:200]):
        j = pos - 1
        while v2[j] != orig:
            assert k2[j] == k2[pos] and orig < v2[j] < v2[pos]
            j -= 1
        assert k2[j] == k2[pos]
