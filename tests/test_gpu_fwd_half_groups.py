"""-m gpu: the forward tile kernel's EIGHT-LANE groups (hsr_render_fwd.hip, the per-lane kernels: K = 0, 16, 26, the 32-channel chunk and the
non-semantic variant) against the CPU oracle.

Every 8-lane group of a wave owns a 4x2 half-block (four pixels wide, two high) and walks a list of its own, which the wave builds from the
half masks staged with each batch (hsr_tile_common.h: subblock_half_mask, build_half_lists); the 16-bit sub-block mask the backward reads
is what it was.  The scenes are hand-placed with the conventions of test_gpu_fwd_visit_stages.py (whose scene builder and checker are used
here), or random where the issue is the image size or the number of batches, and each is aimed at something the halves can break:

  1. a splat whose alpha >= 1/255 region crosses a 4x4 sub-block only between its pixel rows 1 and 2 — the sub-block's bit is set and
     neither half is reached — between contributing entries of the same sub-block, in every sub-block row of the tile (top and bottom
     included) and every column;
  2. a splat that reaches exactly one half of one sub-block, for each of the 32 halves of a tile: once one entry per half, once 0 .. 4
     entries per half, so that the eight lists of a wave differ in length and the shorter ones are padded;
  3. splats covering the whole tile: thirty-two full, equal lists;
  4. image heights 33, 34, 35, 40 and widths 49, 50: last tiles of 1, 2, 3 and 8 valid pixel rows, half-blocks cut by the image's edge;
  5. tile lists of two and three batches (3 000 Gaussians on 64x48) under every instantiation, and a half-block whose list is empty in
     the second batch but not in the first;
  6. the median crossing and the last contributor on the first and on the last entry of a half-block's list, beside longer lists in
     the same wave.

The hand-placed scenes are built so that the oracle flags no tie-risk pixel (asserted), and n_contrib and median_pos are compared exactly
on every pixel; on the random scenes they are compared exactly on every pixel the oracle does not flag, and everything else goes
through test_gpu_parity.py's tiers.  What each hand-placed scene was built to do is asserted on the oracle's state."""
import numpy as np
import pytest

import scenes
from harness import run_gpu, run_oracle
from test_gpu_fwd_visit_stages import _check, _depths, _scene, _upstream, _wide
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

KS = [0, 16, 26, 5]                          # 5: rendered by the 32-channel instantiation
BATCH = {0: 240, 16: 212, 26: 224, 5: 200}   # splats staged per batch by the instantiation that serves K


# ---- placing splats on halves.  Half (row hr, column c) of a tile: pixels 4c .. 4c + 3 of pixel rows 2 hr and 2 hr + 1; a pixel's centre
# sits at i + 0.5 in image coordinates, so the half's centre is (4c + 2, 2 hr + 1) ----
def _on_half(hr, c, z, opacity=0.03, x0=0.0, y0=0.0):
    """sigma 0.4 px (0.68 after the 0.3 px^2 low-pass) at the half's centre: at opacity 0.03 alpha reaches 1/255 within 1.4 px, short of the
    pixel rows above and below the half (1.5 px) and of the columns beside it (2.5 px); the half's four inner pixels see 0.58 x the
    opacity.  Opacity 0.99 reaches 2.3 px: the halves above and below as well."""
    return (x0 + 4.0 * c + 2.0, y0 + 2.0 * hr + 1.0, z, 0.4, 0.4, opacity)


def _in_gap(y_line, c, z, x0=0.0, y0=0.0):
    """opacity 0.0045 (255 o = 1.15), sigma_y 0.05 (0.55 after the low-pass), sigma_x 1: alpha >= 1/255 only within 0.29 px of the line
    y = y_line and 0.55 px of the column's middle, the test's margins included under 0.35: on an integer line no pixel centre is reached"""
    return (x0 + 4.0 * c + 2.0, y0 + float(y_line), z, 1.0, 0.05, 0.0045)


def gaps(K, seed=31):
    """every sub-block of the tile: a contributing splat on each of its halves, a splat in the gap between the sub-block's pixel rows 1 and 2
    behind them, and a contributing splat on each half again behind that"""
    r = np.random.RandomState(seed)
    z = _depths(5 * 16, r)
    out, i = [], 0
    for sr in range(4):
        for c in range(4):
            out += [_on_half(2 * sr, c, z[i]), _on_half(2 * sr + 1, c, z[i + 1]), _in_gap(4 * sr + 2, c, z[i + 2]),
                    _on_half(2 * sr, c, z[i + 3]), _on_half(2 * sr + 1, c, z[i + 4])]
            i += 5
    order = r.permutation(len(out))   # list order = depth order: the z values are dealt out again
    zs = sorted(s[2] for s in out)
    return [out[j][:2] + (zs[k],) + out[j][3:] for k, j in enumerate(order)]


def one_per_half(K, seed=32):
    r = np.random.RandomState(seed)
    z = _depths(32, r)
    where = [(hr, c) for hr in range(8) for c in range(4)]
    r.shuffle(where)
    return [_on_half(hr, c, z[i]) for i, (hr, c) in enumerate(where)]


def uneven_halves(K, seed=33):
    """half (hr, c) gets (3 hr + c) % 5 entries: the eight lists of every wave differ, some are empty"""
    r = np.random.RandomState(seed)
    where = [(hr, c) for hr in range(8) for c in range(4) for _ in range((3 * hr + c) % 5)]
    r.shuffle(where)
    z = _depths(len(where), r)
    return [_on_half(hr, c, z[i]) for i, (hr, c) in enumerate(where)]


def whole_tile(K, n=40, seed=34):
    r = np.random.RandomState(seed)
    z = _depths(n, r)
    return [_wide(z[i], r, 0.05) for i in range(n)]


def half_seam(K, seed=35):
    """the eight halves of wave 0 in turn through the first batch, whose last entry is on half (0, 0); the three entries of the second batch
    are all on half (0, 0): the other seven lists of the wave are empty there, and so are all lists of the other waves"""
    r = np.random.RandomState(seed)
    B = BATCH[K]
    z = _depths(B + 3, r)
    halves = [(hr, c) for hr in range(4) for c in range(2)]
    return [_on_half(*((0, 0) if i >= B - 1 else halves[i % 8]), z[i], opacity=0.02) for i in range(B + 3)]


def ends(K, which, seed=36):
    """half (1, 0) of wave 0 under a list of twelve entries, beside a list of twenty on half (2, 1) and one of three on half (0, 1):
       first_only   one opaque entry in front (alpha 0.57 on the inner pixels: T crosses 0.5), then eleven gap entries on the line between the
                    half's two pixel rows — on its list, reaching no pixel: median and last contributor are the list's FIRST entry;
       last_only    eleven gap entries, then the opaque one: both are the list's LAST entry;
       first_last   the opaque entry, then eleven faint ones: the median on the first entry, the last contributor on the last;
       faint_last   eleven faint entries (T stays above 0.8), then the opaque one: both on the last entry, behind contributions."""
    r = np.random.RandomState(seed)
    n = 12 + 20 + 3
    z = _depths(n, r)
    mine = sorted(r.choice(n, 12, replace=False).tolist())   # list positions of half (1, 0)'s entries among the tile's
    others = [p for p in range(n) if p not in mine]
    out = [None] * n
    for k, p in enumerate(others):
        out[p] = _on_half(2, 1, z[p]) if k < 20 else _on_half(0, 1, z[p])
    strong, gap, faint = (lambda p: _on_half(1, 0, z[p], opacity=0.99)), (lambda p: _in_gap(3, 0, z[p])), (lambda p: _on_half(1, 0, z[p], opacity=0.03))
    kinds = {"first_only": [strong] + [gap] * 11, "last_only": [gap] * 11 + [strong], "first_last": [strong] + [faint] * 11,
             "faint_last": [faint] * 11 + [strong]}[which]
    for k, p in enumerate(mine):
        out[p] = kinds[k](p)
    return out, mine


SCENES = {
    "gaps": lambda K: (16, 16, gaps(K)),
    "one_per_half": lambda K: (16, 16, one_per_half(K)),
    "uneven_halves": lambda K: (16, 16, uneven_halves(K)),
    "whole_tile": lambda K: (16, 16, whole_tile(K)),
    "half_seam": lambda K: (16, 16, half_seam(K)),
    "ends_first_only": lambda K: (16, 16, ends(K, "first_only")[0]),
    "ends_last_only": lambda K: (16, 16, ends(K, "last_only")[0]),
    "ends_first_last": lambda K: (16, 16, ends(K, "first_last")[0]),
    "ends_faint_last": lambda K: (16, 16, ends(K, "faint_last")[0]),
}


def _half_of(n, hr, c):
    return n[2 * hr:2 * hr + 2, 4 * c:4 * c + 4]


def expectations(name, K, st, splats):
    """what the scene was built to do, asserted on the ORACLE's state (so it can be checked without a GPU)"""
    n, med = st["n_contrib"], st["median_pos"]
    if name in ("gaps", "one_per_half", "uneven_halves"):
        # a pixel's last contributor is an entry placed on ITS half, and every half's last entry is some pixel's last contributor
        last = {}
        for i, s in enumerate(splats):
            if s[5] > 0.0045:   # not a gap entry
                last[(int((s[1] - 1.0) // 2), int((s[0] - 2.0) // 4))] = i + 1
        for hr in range(8):
            for c in range(4):
                blk = _half_of(n, hr, c)
                own = {i + 1 for i, s in enumerate(splats) if s[5] > 0.0045 and (int((s[1] - 1.0) // 2), int((s[0] - 2.0) // 4)) == (hr, c)}
                assert set(blk.reshape(-1).tolist()) - {0} <= own, (hr, c)
                assert blk.max() == last.get((hr, c), 0), (hr, c)
        if name == "gaps":
            assert sum(s[5] == 0.0045 for s in splats) == 16 and len(last) == 32
    elif name == "whole_tile":
        assert (n == len(splats)).all()
    elif name == "half_seam":
        B = BATCH[K]
        assert _half_of(n, 0, 0).max() == B + 3
        rest = n.copy()
        rest[:2, :4] = 0
        assert 0 < rest[:8, :8].max() <= B - 1 and rest[8:, :].max() == 0 and rest[:, 8:].max() == 0
    elif name.startswith("ends"):
        mine = ends(K, name[5:])[1]
        blk_n, blk_m = _half_of(n, 1, 0)[:, 1:3], _half_of(med, 1, 0)[:, 1:3]   # the half's four inner pixels
        first, last = mine[0] + 1, mine[-1] + 1
        want_med, want_last = {"first_only": (first, first), "last_only": (last, last), "first_last": (first, last),
                               "faint_last": (last, last)}[name[5:]]
        assert (blk_m == want_med).all() and (blk_n == want_last).all(), (blk_m, blk_n, want_med, want_last)
        assert _half_of(n, 2, 1).max() > 0 and _half_of(n, 0, 1).max() > 0


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", list(SCENES))
def test_half_groups(name, K):
    W, H, splats = SCENES[name](K)
    cam, sc = _scene(W, H, K, splats)
    expectations(name, K, _check(cam, sc, _upstream(W, H, K)), splats)


@pytest.mark.parametrize("name", ["gaps", "uneven_halves", "half_seam", "ends_first_last"])
def test_half_groups_non_semantic(name):
    W, H, splats = SCENES[name](0)
    cam, sc = _scene(W, H, 0, splats)
    expectations(name, 0, _check(cam, sc, _upstream(W, H, 0), semantic=False), splats)


@pytest.mark.parametrize("top", [0, 1])
def test_gap_rows_of_neighbouring_tiles(top):
    """the gap splats of scene 1 in the top sub-block row of the lower tile and the bottom sub-block row of the upper one (image 16x32), with
    contributing splats on the halves around them"""
    r = np.random.RandomState(37 + top)
    y0 = 16.0 * top
    rows = [0] if top else [3]
    z = _depths(3 * 4 * len(rows), r)
    splats, i = [], 0
    for sr in rows:
        for c in range(4):
            splats += [_on_half(2 * sr, c, z[i], y0=y0), _in_gap(4 * sr + 2, c, z[i + 1], y0=y0), _on_half(2 * sr + 1, c, z[i + 2], y0=y0)]
            i += 3
    cam, sc = _scene(16, 32, 26, splats)
    st = _check(cam, sc, _upstream(16, 32, 26))
    n = st["n_contrib"]
    band = n[int(y0) + 4 * rows[0]:int(y0) + 4 * rows[0] + 4]
    assert band.max() > 0 and n.sum() == band.sum()
    assert not np.isin(band, [i + 1 for i, s in enumerate(splats) if s[5] == 0.0045]).any()


# ---- random scenes: the image's edge, and lists of two and three batches ----
def _ints_exact_off_ties(cam, sc, up, semantic=True):
    """n_contrib and median_pos, bit for bit on every pixel the oracle does not flag as a tie risk; returns the tile lists' lengths"""
    out_o, gr_o, st_o = run_oracle(cam, sc, up, semantic=semantic)
    try:
        out_g, gr_g, st_g = run_gpu(cam, sc, up, semantic=semantic, want_state=True)
        keep = ~np.asarray(st_o.field("tie_pixels")).astype(bool).reshape(-1)
        assert keep.mean() > 0.9
        for nme in ("n_contrib", "median_pos"):
            e, g = np.asarray(st_o.field(nme)).reshape(-1).astype(np.uint32), np.asarray(st_g[nme]).reshape(-1)
            bad = (g != e) & keep
            assert not bad.any(), "%s differs on %d unflagged pixels, first at %d: %d vs %d" % (
                nme, int(bad.sum()), int(np.argmax(bad)), int(g[np.argmax(bad)]), int(e[np.argmax(bad)]))
        rng = np.asarray(st_o.field("ranges")).reshape(-1, 2).astype(np.int64)
        return rng[:, 1] - rng[:, 0]
    finally:
        st_o.free()


@pytest.mark.parametrize("W,H", [(49, 33), (50, 34), (49, 35), (50, 40)])
def test_image_edges(W, H):
    """last tiles with 1, 2, 3 and 8 valid pixel rows and 1 and 2 valid columns: half-blocks cut by the image's edge"""
    cam, sc, up = scenes.build(W, H, 700, 26, seed=41, kind="aniso", scale_mult=2.0)
    _ints_exact_off_ties(cam, sc, up)
    _compare(cam, sc, up, True, "sr")


# tile lists of 350 .. 400 entries (2 000 Gaussians: two batches under every instantiation) and of 510 .. 580 (3 000: three batches)
MULTI = {2: dict(W=64, H=48, P=2000, seed=43, kind="aniso", scale_mult=1.2), 3: dict(W=64, H=48, P=3000, seed=43, kind="aniso", scale_mult=1.2)}


def _multi(batches, K):
    m = MULTI[batches]
    return scenes.build(m["W"], m["H"], m["P"], K, seed=m["seed"], kind=m["kind"], scale_mult=m["scale_mult"])


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("batches", [2, 3])
def test_two_and_three_batches(batches, K):
    cam, sc, up = _multi(batches, K)
    n = _ints_exact_off_ties(cam, sc, up)
    B = BATCH[K]
    assert ((n > (batches - 1) * B) & (n <= batches * B)).all(), "every tile must stage %d batches of %d: %s" % (batches, B, n)
    _compare(cam, sc, up, True, "sr")


@pytest.mark.parametrize("batches", [2, 3])
def test_two_and_three_batches_non_semantic(batches):
    cam, sc, up = _multi(batches, 0)
    n = _ints_exact_off_ties(cam, sc, up, semantic=False)
    assert ((n > (batches - 1) * 240) & (n <= batches * 240)).all(), n
    _compare(cam, sc, up, False, "sr")
