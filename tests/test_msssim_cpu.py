"""CPU suite for the multi-scale SSIM: the checker's two float64 restatements (tests/msssim_ref.py) agree, identical images score
exactly 1, a pool without the front padding is told apart, and the prototypes of include/ext/hsr_msssim.h are exported and bound
with the header's types (the checker of tests/test_abi.py, pointed at the extension header)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import msssim_ref as R
import test_abi

EXT_HEADER = os.path.join(test_abi.ROOT, "include", "ext", "hsr_msssim.h")
CASES = R.cases()


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


def test_msssim_abi_exported_and_bound(monkeypatch):
    from diff_gaussian_rasterization import _C, _abi
    monkeypatch.setattr(test_abi, "HEADERS", [EXT_HEADER])
    protos = test_abi._prototypes()
    assert sorted(protos) == sorted(s[0] for s in _abi.SIGNATURES_EXT) == ["hsr_eval_msssim", "hsr_eval_msssim_scratch_bytes"]
    assert [s[0] for s in _abi.SIGNATURES_EXT] == list(protos)      # in the header's order
    lib = C.CDLL(_C._LIB_PATH)
    for name, proto in protos.items():
        assert hasattr(lib, name), "libhsr_rast.so does not export %s" % name
        test_abi.check_signature(name, proto)
    assert not {s[0] for s in _abi.SIGNATURES} & set(protos)


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
