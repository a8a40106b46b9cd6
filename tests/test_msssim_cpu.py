"""CPU suite for the multi-scale SSIM: the checker's two float64 restatements (tests/msssim_ref.py) agree, identical images score
exactly 1, a pool without the front padding is told apart, and the prototypes of include/ext/hsr_msssim.h are the two named
here (tests/test_abi.py checks that they are exported and bound with the header's types).

For the tile suite (tests/test_gpu_msssim_tiles.py) it also holds the conditions on that suite's inputs that need no GPU: the scratch
size equals the restated layout, the sizes reach every class of last tile and level parity, the explicit-slice maps reproduce the
float64 reference, and a deliberately wrong restatement (one changed pixel of any level; a pool without the front padding) moves a tile sum past the
tile budget."""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import msssim_ref as R
import test_abi

EXT_HEADER = "ext/hsr_msssim.h"
CASES = R.cases()
TILE_CASES = R.tile_cases()


def _inputs(case):
    im, gt, depth, opacity, thres, _score, _table = R.reference(case)
    return R.masked(im, gt, depth, opacity if case[4] else None, thres)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatements_agree(case):
    x, y = _inputs(case)
    score_t, table_t = R.reference(case)[5:]
    score_s, table_s = R.msssim_scipy(x.numpy(), y.numpy())
    assert abs(score_t - score_s) <= 1e-12, (score_t, score_s)
    assert np.abs(table_t - table_s).max() <= 1e-12
    assert 0.0 < score_t < 1.0 and np.abs(table_t).max() <= 1.0


@pytest.mark.parametrize("H,W", R.SMALL_SIZES)
def test_identical_images_score_one(H, W):
    im = R.make_frame(H, W, "texture", seed=1)[0]
    for score, table in (R.msssim_torch(im, im, torch.float64), R.msssim_scipy(im.numpy(), im.numpy())):
        assert score == 1.0
        assert (table == 1.0).all()


@pytest.mark.parametrize("case", [c for c in CASES if (c[1] % 2 or c[2] % 2) and not c[4]], ids=lambda c: c[0])
def test_floor_pooling_is_told_apart(case):
    """negative control: dropping the odd row / column instead of padding in front of it moves at least one per-scale mean by more than
    1e-3 (ten times the GPU suite's bound); scales the floor pyramid cannot reach (a side under 11) are not compared"""
    x, y = _inputs(case)
    table = R.reference(case)[6]
    _score, floor_table = R.msssim_torch(x, y, torch.float64, pool_padding=False)
    assert np.isfinite(floor_table[:4]).all()
    dist = np.nanmax(np.abs(floor_table - table))
    print("%s: floor pooling moves a per-scale mean by %.3e" % (case[0], dist))
    assert dist > 1e-3


def test_msssim_abi_exported_and_bound():
    from diff_gaussian_rasterization import _abi
    protos = test_abi._prototypes([EXT_HEADER])
    assert sorted(protos) == sorted(s[0] for s in _abi.HEADERS[EXT_HEADER]) == ["hsr_eval_msssim", "hsr_eval_msssim_scratch_bytes"]
    assert [s[0] for s in _abi.HEADERS[EXT_HEADER]] == list(protos)      # in the header's order


def test_python_limits_equal_header_defines():
    from hsr_utils import evaluate as E
    defines = {m.group(1): int(m.group(2))
               for m in re.finditer(r"^#define\s+(HSR_\w+)\s+\(?(-?\d+)\)?\s*$", test_abi._source(EXT_HEADER), flags=re.M)}
    assert E.MSSSIM_MIN_SIDE == defines["HSR_EVAL_MSSSIM_MIN_SIDE"] == 161
    assert E.MSSSIM_SCALES == defines["HSR_EVAL_MSSSIM_SCALES"] == len(R.WEIGHTS)
    assert E.MSSSIM_OUT == defines["HSR_EVAL_MSSSIM_OUT"] == 1 + 5 * 3 * 2


def test_host_only_entry_points():
    """sizes are answered and illegal ones refused before any device work"""
    from hsr_utils import evaluate as E
    lib = E._lib

    def pyramid_floats(H, W):
        n = 0
        for _ in range(4):
            H, W = (H + 1) // 2, (W + 1) // 2
            n += 6 * H * W
        return n

    for H, W in R.SMALL_SIZES + (R.LARGE_SIZE,):
        assert lib.hsr_eval_msssim_scratch_bytes(H, W) > 4 * pyramid_floats(H, W)
    for H, W in ((160, 400), (400, 160), (0, 0), (161, -5)):
        assert lib.hsr_eval_msssim(H, W, *([None] * 4), 0.0, None, None, 0, None) == -1
        assert b"eval_msssim" in lib.hsr_last_error() and b"160" in lib.hsr_last_error()
    assert lib.hsr_eval_msssim(161, 161, *([None] * 4), 0.0, None, None, 0, None) == -1      # NULL images


def test_cpu_tensors_and_small_images_are_refused():
    from hsr_utils import evaluate as E
    x = torch.zeros(3, 200, 200)
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.ms_ssim(x, x, x[0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.evaluate_frame(x, x, x[0], x[0], x, x[0].int(), "flat", num_classes=3, ms_ssim=True)


# ---------------------------------------------------------------- conditions on the tile suite's inputs
def test_scratch_bytes_equal_the_restated_layout():
    from hsr_utils import evaluate as E
    for H, W in sorted({(c[1], c[2]) for c in TILE_CASES + CASES}):
        lay = R.scratch_layout(H, W)
        assert E._lib.hsr_eval_msssim_scratch_bytes(H, W) == lay["bytes"], (H, W)
        assert lay["part_base"] % 256 == 0 and lay["bytes"] % 256 == 0
        assert lay["part_base"] - 4 * lay["pyr_floats"] < 256 and lay["bytes"] - lay["part_base"] - 8 * lay["part_doubles"] < 256
    lay = R.scratch_layout(161, 170)
    assert lay["sizes"] == [(161, 170), (81, 85), (41, 43), (21, 22), (11, 11)]
    assert lay["tiles"] == [(5, 5), (3, 3), (1, 2), (1, 1), (1, 1)]
    assert lay["pyr"] == {1: 0, 2: 6 * 81 * 85, 3: 6 * (81 * 85 + 41 * 43), 4: 6 * (81 * 85 + 41 * 43 + 21 * 22)}
    assert lay["part"] == [0, 150, 204, 216, 222] and lay["part_doubles"] == 228


@pytest.mark.parametrize("axis", (0, 1), ids=("rows", "columns"))
def test_tile_sizes_cover_every_class(axis):
    """on each axis, at level 0 and again at a level 1 to 3: the last tile owns 42 (even size, (n - 10) % 32 == 0), has one output
    (odd, == 1) or 31 (odd, == 31), plus another even and another odd size; and some level is exactly 42: a single tile that owns
    everything"""
    sizes = [R.level_sizes(c[1], c[2]) for c in TILE_CASES]
    level0 = {lv[0][axis] for lv in sizes}
    deeper = {lv[s][axis] for lv in sizes for s in (1, 2, 3)}
    for name, where in (("level 0", level0), ("levels 1 to 3", deeper)):
        rest = lambda n: (n - 10) % 32
        assert any(n % 2 == 0 and rest(n) == 0 for n in where), name
        assert any(n % 2 == 1 and rest(n) == 1 for n in where), name
        assert any(n % 2 == 1 and rest(n) == 31 for n in where), name
        assert any(n % 2 == 0 and rest(n) != 0 for n in where), name
        assert any(n % 2 == 1 and rest(n) not in (1, 31) for n in where), name
    assert 42 in deeper


@pytest.mark.parametrize("case", TILE_CASES, ids=[c[0] for c in TILE_CASES])
def test_tile_reference_restates_the_float64_reference(case):
    """the explicit-slice maps, summed tile by tile, give the table and the score of msssim_torch in float64; the explicit pool gives
    avg_pool2d's levels.  The float32 restatement's own tile sums stay within 0.7 of the budget: with m = 4 that follows from
    |sum32 - sum64| <= L1 = budget / 4 and says nothing about float32; it only guards the bookkeeping (sums, L1 and budget taken
    from the same maps and tiles)"""
    ref = R.tile_reference(case)
    sizes = R.level_sizes(case[1], case[2])
    score64, table64 = R.reference(case)[5:]
    table = R.table_of(ref["tiles64"], sizes)
    assert np.abs(table - table64).max() <= 1e-12
    assert abs(R.score_of(table) - score64) <= 1e-12
    x = ref["x"].double()[None]
    for s in range(1, 5):
        x = F.avg_pool2d(x, 2, padding=[n % 2 for n in x.shape[2:]])
        assert tuple(x.shape[2:]) == sizes[s] == tuple(ref["levels64"][s][0].shape[1:])
        assert (x[0] - ref["levels64"][s][0]).abs().max() <= 1e-15
    for s in range(5):
        assert ref["tiles64"][s].shape == (3, 2) + R.scratch_layout(case[1], case[2])["tiles"][s]
        assert ref["pixels"][s].sum() == (sizes[s][0] - 10) * (sizes[s][1] - 10)
        own = (ref["tiles32"][s] - ref["tiles64"][s]).abs()
        assert (own <= 0.7 * ref["budget"][s]).all()


def _seam_pixel(h, w):
    """an image pixel whose 11x11 footprint in the map straddles the seam between the first two tiles (map row / column 31 | 32 is
    image row / column 36 | 37) on every axis that has one, else the middle"""
    return (37 if h - 10 > R.TILE else h // 2), (37 if w - 10 > R.TILE else w // 2)


@pytest.mark.parametrize("case", TILE_CASES, ids=[c[0] for c in TILE_CASES])
def test_one_changed_pixel_moves_a_tile_sum_past_the_budget(case):
    """teeth of the tile budget: at every scale, adding 0.5 mod 1 to ONE pixel of that level's x image moves at least one float64
    tile sum by more than the budget the GPU suite grants the kernel there"""
    ref = R.tile_reference(case)
    for s, (xs, ys) in enumerate(ref["levels64"]):
        r, c = _seam_pixel(*xs.shape[1:])
        xs = xs.clone()
        xs[s % 3, r, c] = (xs[s % 3, r, c] + 0.5) % 1
        moved = (R.tile_sums(torch.stack(R.level_maps(xs, ys), 1)) - ref["tiles64"][s]).abs()
        ratio = (moved / ref["budget"][s]).max().item()
        print("%s scale %d: pixel (%d, %d, %d) moves a tile sum by %.3e, %.0f times its budget" % (case[0], s, s % 3, r, c, moved.max(), ratio))
        assert ratio > 1.0, (s, ratio)
        assert (moved > 0).sum() <= 4 * 2, "one pixel reaches at most the four tiles around a seam crossing, in one channel"


@pytest.mark.parametrize("case", [c for c in TILE_CASES if c[1] < 680], ids=lambda c: c[0])
def test_floor_pooling_is_told_apart_below_the_means(case):
    """negative control of the pyramid and tile checks (every size of TILE_SIZES is odd at level 0 or 1 on some axis): a pool that
    drops the odd row / column instead of padding in front of it gives a float32 pyramid that differs from the padded one in shape or
    bits from the first level pooled from an odd one, and maps whose tile sums leave the budget, or whose tile grid changes, at some
    scale of 1 or above"""
    ref = R.tile_reference(case)
    sizes = R.level_sizes(case[1], case[2])
    first = next(s for s in range(1, 5) if sizes[s - 1][0] % 2 or sizes[s - 1][1] % 2)
    good, floor = R.pyramid_fp32(ref["x"], ref["y"]), R.pyramid_fp32(ref["x"], ref["y"], pool_padding=False)
    for s in range(1, 5):
        same = all(g.shape == f.shape and torch.equal(g, f) for g, f in zip(good[s - 1], floor[s - 1]))
        assert same == (s < first), s
    told = []
    for s, maps in enumerate(R.scale_maps(ref["x"], ref["y"], torch.float64, pool_padding=False)):
        if min(maps[0].shape[1:]) < 1:      # the floor pyramid's last level can fall under 11
            told.append("scale %d: no map" % s)
            continue
        sums = R.tile_sums(torch.stack(maps, 1))
        if sums.shape != ref["tiles64"][s].shape:
            told.append("scale %d: tile grid %s, not %s" % (s, tuple(sums.shape[2:]), tuple(ref["tiles64"][s].shape[2:])))
        elif ((sums - ref["tiles64"][s]).abs() > ref["budget"][s]).any():
            told.append("scale %d: %.1e times the budget" % (s, ((sums - ref["tiles64"][s]).abs() / ref["budget"][s]).max()))
        else:
            assert s < first, s
    print("%s: %s" % (case[0], "; ".join(told)))
    assert told and all(int(t.split()[1][:-1]) >= first for t in told)
