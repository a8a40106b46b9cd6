"""CPU suite for the edge cases of the densify select (tests/depth_error_cases.py), torch CPU ops alone:
    every case sits in the regime it is named for (else tests/test_gpu_densify_frame_edges.py could pass without reaching that edge);
    oracle/densify_oracle.non_presence_points gives the reference's median (bit for bit, NaN by NaN) and mask (bit for bit) on every case,
    the reference's expressions being tests/test_densify.torch_reference (scripts/hierslam.py:1271-1278, :1289-1290)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import depth_error_cases as DC
from test_densify import torch_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import densify_oracle as DO  # noqa: E402

HIST_VALUES, MASK_BLOCK = 2048, 256      # values per histogram workgroup and pixels per mask block of csrc/hsr_densify.hip


def _bits(t):
    return torch.as_tensor(t).reshape(-1).view(torch.int32)


def _same_bits(got, want):
    """bit-equal, where every NaN counts as the same NaN"""
    g, w = torch.as_tensor(got).reshape(-1), torch.as_tensor(want).reshape(-1)
    return bool(((_bits(g) == _bits(w)) | (torch.isnan(g) & torch.isnan(w))).all())


@functools.lru_cache(maxsize=None)
def _error_and_median(case):
    rd, gt = DC.ALL_CASES[case]()
    e = torch.abs(gt - rd) * (gt > 0)
    return e.reshape(-1), e.median()


def _byte(x, b):
    return (int(_bits(x)[0]) >> (8 * b)) & 255


@pytest.mark.parametrize("case,byte,median_bits", [("byte0_only", 0, 0x3f80007f), ("byte1_only", 1, 0x3f807f00), ("byte2_only", 2, 0x3f7f0000),
                                                   ("byte3_only", 3, 0x3f000000)])
def test_byte_cases_differ_in_one_byte(case, byte, median_bits):
    e, median = _error_and_median(case)
    keys = _bits(e).tolist()
    n = len(keys)
    assert len(set(keys)) == n and len({(k >> (8 * byte)) & 255 for k in keys}) == n           # all different, in that byte alone
    assert len({k & ~(255 << (8 * byte)) for k in keys}) == 1
    assert bool(torch.isfinite(e).all()) and bool((e >= 0).all())
    assert int(_bits(median)[0]) == median_bits and _byte(median, byte) == (n - 1) // 2
    assert case != "byte3_only" or (n == 128 and _byte(median, 3) == 63)


@pytest.mark.parametrize("case,byte", [("bucket255_byte0", 0), ("bucket255_byte1", 1), ("bucket255_byte2", 2)])
def test_bucket_255_cases_end_the_pick_loop(case, byte):
    """the median's byte is 0xff, five of nine values equal it, and in that pass the candidates (the values that share the higher bytes) below
    it are fewer than the rank: the pick loop runs through buckets 0 .. 254 without a hit"""
    e, median = _error_and_median(case)
    m = int(_bits(median)[0])
    assert _byte(median, byte) == 0xff and e.numel() == 9 and int((e == median).sum()) == 5
    high = ~((1 << (8 * (byte + 1))) - 1)
    candidates = [k for k in _bits(e).tolist() if k & high == m & high]
    below = [k for k in candidates if (k >> (8 * byte)) & 255 < 255]
    rank_in_pass = 4 - sum(1 for k in _bits(e).tolist() if k & high < m & high)
    assert len(below) <= rank_in_pass < len(candidates) and len(below) == 2
    assert torch.equal(median, e.sort().values[4])


def test_special_medians():
    """0, inf and NaN medians, and what feeds them"""
    for case in ("1x1_hole", "5x7_18_holes"):
        assert float(_error_and_median(case)[1]) == 0.0
    e, median = _error_and_median("mostly_inf_errors")
    rd, gt = DC.ALL_CASES["mostly_inf_errors"]()
    assert float(median) == DC.INF and int((e == DC.INF).sum()) == 8 > e.numel() // 2 and bool((gt > 0).all())
    assert not bool(((rd > gt).reshape(-1) & (e > 50 * median)).any())                                 # threshold inf: nothing is greater
    nan_cases = ("nan_depth_valid_pixel", "nan_depth_under_hole", "inf_depth_under_hole", "nan_gt", "1x7_inf_over_hole", "nan_turns_depth_mask_off",
                 "3x683_nan_last_pixel")
    for case in DC.ALL_CASES:
        e, median = _error_and_median(case)
        assert bool(torch.isnan(median)) == (case in nan_cases) == bool(torch.isnan(e).any()), case
    # what a rank rule without the NaN rule makes of them: a finite median; in two cases it would switch the depth part of the mask on
    for case in nan_cases:
        e = _error_and_median(case)[0]
        assert bool(torch.isfinite(torch.nan_to_num(e, nan=DC.INF).sort().values[(e.numel() - 1) // 2])), case
    assert int(torch.isnan(_error_and_median("nan_gt")[0]).sum()) == 1 and bool(torch.isnan(DC.ALL_CASES["nan_gt"]()[1]).any())
    e = _error_and_median("1x7_inf_over_hole")[0]
    assert float(e.nan_to_num(nan=DC.INF).sort().values[3]) == pytest.approx(0.1)              # the worked example: 0.1 by rank, NaN by torch
    rd, gt = DC.ALL_CASES["nan_turns_depth_mask_off"]()
    e = _error_and_median("nan_turns_depth_mask_off")[0]
    by_rank = e.nan_to_num(nan=DC.INF).sort().values[3]
    assert float(by_rank) == 2.0 ** -10 and ((rd > gt).reshape(-1) & (e > 50 * by_rank)).tolist() == [False] * 6 + [True]
    e = _error_and_median("3x683_nan_last_pixel")[0]
    assert torch.isnan(e).nonzero().tolist() == [[2048]]                                      # alone in the second histogram workgroup


def test_frame_sizes_sit_on_the_select_s_edges():
    size = {c: DC.ALL_CASES[c]()[1].numel() for c in ("23x89", "32x64", "3x683", "512x512", "513x512")}
    assert [size[c] for c in ("23x89", "32x64", "3x683")] == [HIST_VALUES - 1, HIST_VALUES, HIST_VALUES + 1]
    assert [-(-size[c] // HIST_VALUES) for c in ("23x89", "32x64", "3x683")] == [1, 1, 2]
    blocks = {c: -(-n // MASK_BLOCK) for c, n in size.items()}
    assert blocks["512x512"] == 1024 and size["512x512"] % MASK_BLOCK == 0 and blocks["513x512"] == 1026     # one, then two counts per scan thread
    for c in size:                  # a finite, non-zero median, and a depth part of the mask that is neither empty nor everything
        e, median = _error_and_median(c)
        rd, gt = DC.ALL_CASES[c]()
        by_depth = ((rd > gt) & (e.reshape(gt.shape) > 50 * median) & (gt > 0))
        assert 0 < float(median) < 0.1 and 0 < int(by_depth.sum()) < 0.05 * size[c], c


def _frames():
    out = [("case:" + c, functools.partial(DC.densify_frame, c), 50) for c in DC.ALL_CASES]
    out += [("comparisons:%s%s" % (f, ":nan_gt" if n else ""), functools.partial(lambda f, n: DC.comparison_frame(f, n)[0], f, n), f)
            for f in (50, 12.5) for n in (False, True)]
    out += [("emission:" + w, functools.partial(DC.emission_frame, w), 50) for w in DC.EMISSION_MASKS]
    return out


@pytest.mark.parametrize("name,build,factor", _frames(), ids=[f[0] for f in _frames()])
def test_oracle_median_and_mask_equal_the_reference_expressions(name, build, factor):
    sil, rd, gt, col, K, w2c = build()
    ref = torch_reference(sil, rd, gt, col, K, w2c, DC.SIL_THRES, depth_factor=factor, full=True)
    o = DO.non_presence_points(sil.numpy(), rd.numpy(), gt.numpy(), col.numpy(), K.numpy(), torch.inverse(w2c).numpy(), DC.SIL_THRES, depth_factor=factor)
    assert _same_bits(torch.tensor(np.float32(o["median"])), ref["median"]), (name, o["median"], ref["median"])
    assert o["mask"].dtype == np.bool_ and np.array_equal(o["mask"], ref["mask"].numpy()), name
    assert o["means3D"].shape == (int(ref["mask"].sum()), 3)


def test_comparison_and_emission_frames_are_what_they_claim():
    for factor in (50, 12.5):
        for nan_gt in (False, True):
            frame, expect = DC.comparison_frame(factor, nan_gt)
            ref = torch_reference(*frame, DC.SIL_THRES, depth_factor=factor, full=True)
            assert torch.equal(ref["mask"], expect), (factor, nan_gt)
            if nan_gt:
                assert bool(torch.isnan(ref["median"]))
                continue
            e = ref["depth_error"].reshape(-1)
            assert float(ref["median"]) == 2.0 ** -10 and float(ref["threshold"]) == factor * 2.0 ** -10
            assert float(e[7]) == float(ref["threshold"]) and float(e[8]) == float(ref["threshold"]) + 2.0 ** -11      # on it, and one step beyond
            assert float(e[6]) == 0.0 and float(e[9]) == 0.5 and float(frame[0].reshape(-1)[10]) == DC.SIL_THRES
            assert float(frame[0].reshape(-1)[11]) < DC.SIL_THRES and float(frame[0].reshape(-1)[11]) > DC.SIL_THRES - 1e-7
    n = 300
    want = {"edges": [63, 64, 255, 256, n - 1], "everywhere": list(range(n)), "nowhere": []}
    for which in DC.EMISSION_MASKS:
        ref = torch_reference(*DC.emission_frame(which), DC.SIL_THRES, full=True)
        assert ref["mask"].nonzero().reshape(-1).tolist() == want[which] and float(ref["median"]) == 0.0


def test_densify_frames_let_the_depth_part_show():
    """up to 16 pixels the silhouette selects nothing, so the mask IS the depth part; the larger frames have both parts"""
    for case in DC.ALL_CASES:
        sil, rd, gt = DC.densify_frame(case)[:3]
        by_sil = (sil < DC.SIL_THRES) & (gt > 0)
        assert bool(by_sil.any()) == (gt.numel() > 16), case
    for case in ("37x23", "129x67", "340x600", "513x512", "512x512", "23x89", "32x64", "3x683"):
        sil, rd, gt, col, K, w2c = DC.densify_frame(case)
        ref = torch_reference(sil, rd, gt, col, K, w2c, DC.SIL_THRES, full=True)
        by_sil = ((sil < DC.SIL_THRES) & (gt > 0)).reshape(-1)
        assert int((ref["mask"] & ~by_sil).sum()) > 0, case                                   # pixels that only the depth part selects
