"""CPU suite: the backward's plan (hsr_plan_backward, include/hsr_rasterizer.h) — accumulation mode, tile kernel, row layout and row
stride for given sizes — against a table worked out by hand from the rules: Q-panel kernel for K <= 27 and subw beyond while
P * stride < 2^30 (32-bit row addressing), else the all-VALU kernel on classic rows; compact rows where the Q-panel kernel runs and
they save a 64-byte line; geometry-only on 16-float rows.  Host arithmetic only: no device, no allocation."""
import ctypes as C
import os
import subprocess
import sys

import pytest

Q, QGEO, SUBW, VALU = range(4)      # HSR_BWD_KERNEL_*
PACKED, LEGACY = 0, 2

# (P, K, geometry-only request) -> (kernel, row layout, row stride in floats), all with packed accumulation.  Every P boundary is the
# largest P with P * stride < 2^30 and the one after it.
TABLE = [
    (1000, 0, 0, Q, 1, 16), (1000, 4, 0, Q, 1, 16),
    (1000, 5, 0, Q, 0, 32), (1000, 11, 0, Q, 0, 32),
    (1000, 12, 0, Q, 1, 32), (1000, 16, 0, Q, 1, 32), (1000, 20, 0, Q, 1, 32),
    (1000, 21, 0, Q, 0, 48), (1000, 26, 0, Q, 0, 48), (1000, 27, 0, Q, 0, 48),
    (1000, 28, 0, SUBW, 0, 64),
    (1000, 74, 0, SUBW, 0, 96),
    (1000, 102, 0, SUBW, 0, 128),
    (1000, 26, 1, QGEO, 0, 16),
    (22369621, 26, 0, Q, 0, 48),
    (22369622, 26, 0, VALU, 0, 48),
    (30000000, 16, 0, Q, 1, 32),
    (33554431, 16, 0, Q, 1, 32),
    (33554432, 16, 0, VALU, 0, 48),
    (67108863, 0, 0, Q, 1, 16),
    (67108864, 0, 0, VALU, 0, 32),
    (11184810, 74, 0, SUBW, 0, 96),
    (11184811, 74, 0, VALU, 0, 96),
    (67108863, 26, 1, QGEO, 0, 16),
]
NOT_GRANTED = (67108864, 26)        # P * 16 = 2^30: the geometry-only request is not granted


def _plan(P, K, geo=0, offered=None):
    from diff_gaussian_rasterization import _abi
    plan = _abi.hsr_backward_plan()
    rc = _abi.lib.hsr_plan_backward(P, K, geo, _abi.HSR_SCRATCH_AS_PLANNED if offered is None else offered, C.byref(plan))
    assert rc == 0, _abi.lib.hsr_last_error()
    return plan


def _minimum_scratch(P, K):
    return P * (16 + 16 * ((K + 5 + 15) // 16)) * 4 + 512


@pytest.mark.parametrize("P,K,geo,kernel,layout,stride", TABLE)
def test_plan_table(P, K, geo, kernel, layout, stride):
    from diff_gaussian_rasterization import _abi
    p = _plan(P, K, geo)
    assert (p.accumulation, p.kernel, p.row_layout, p.row_stride, p.geometry_only) == (PACKED, kernel, layout, stride, geo), (P, K, geo)
    assert p.scratch_bytes == _minimum_scratch(P, K) == _abi.lib.hsr_backward_scratch_bytes(P, K, 0)
    assert p.semantic_alpha == 0        # the exact semantic -> alpha mode is opt-in


def test_geometry_only_is_not_granted_beyond_32_bit_rows():
    P, K = NOT_GRANTED
    p = _plan(P, K, 1)
    assert p.geometry_only == 0
    q = _plan(P, K, 0)                  # the plan is then the full backward's
    assert (p.accumulation, p.kernel, p.row_layout, p.row_stride, p.scratch_bytes) == \
        (q.accumulation, q.kernel, q.row_layout, q.row_stride, q.scratch_bytes)


@pytest.mark.parametrize("P,K,geo", [(P, K, geo) for P, K, geo, *_ in TABLE if P == 1000])
def test_scratch_threshold(P, K, geo):
    """too little scratch on offer is legacy accumulation for that call: the threshold is the rows themselves + 256 bytes to align them"""
    need = _minimum_scratch(P, K)
    p = _plan(P, K, geo, need - 257)
    assert (p.accumulation, p.kernel, p.row_layout, p.row_stride, p.geometry_only, p.scratch_bytes) == (LEGACY, VALU, 0, 0, 0, 0)
    assert _plan(P, K, geo, 0).accumulation == LEGACY
    ample = _plan(P, K, geo)
    p = _plan(P, K, geo, need - 256)
    assert (p.accumulation, p.kernel, p.row_layout, p.row_stride, p.geometry_only, p.scratch_bytes) == \
        (PACKED, ample.kernel, ample.row_layout, ample.row_stride, geo, need)


def test_legacy_mode_plans_the_valu_kernel_without_scratch():
    from diff_gaussian_rasterization import _abi
    assert _abi.lib.hsr_set_backward_mode(LEGACY) == 0
    try:
        for P, K, geo, *_ in TABLE + [NOT_GRANTED + (1,)]:
            p = _plan(P, K, geo)
            assert (p.accumulation, p.kernel, p.row_layout, p.row_stride, p.geometry_only, p.scratch_bytes) == (LEGACY, VALU, 0, 0, 0, 0)
            assert _abi.lib.hsr_backward_scratch_bytes(P, K, 0) == 0
    finally:
        assert _abi.lib.hsr_set_backward_mode(PACKED) == 0


def test_empty_and_invalid_sizes():
    from diff_gaussian_rasterization import _abi
    p = _plan(0, 26, 1)                 # nothing to accumulate: no scratch, nothing granted
    assert (p.accumulation, p.geometry_only, p.scratch_bytes) == (LEGACY, 0, 0) and _abi.lib.hsr_backward_scratch_bytes(0, 26, 0) == 0
    plan = _abi.hsr_backward_plan()
    assert _abi.lib.hsr_plan_backward(-1, 0, 0, 0, C.byref(plan)) == -1 and b"hsr_plan_backward" in _abi.lib.hsr_last_error()
    assert _abi.lib.hsr_plan_backward(10, -1, 0, 0, C.byref(plan)) == -1
    assert _abi.lib.hsr_plan_backward(10, 0, 0, 0, None) == -1


def test_valu_selector_in_a_child_process():
    """HSR_BWD_IMPL=valu (read once per process): the all-VALU kernel on classic packed rows; the geometry-only path keeps its kernel"""
    code = r'''
import ctypes as C, sys
lib = C.CDLL(sys.argv[1])       # the bare library: the child need not import torch
lib.hsr_plan_backward.argtypes = [C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p]
def plan(P, K, geo):
    p = (C.c_int * 8)()         # hsr_backward_plan: six ints, then scratch_bytes
    assert lib.hsr_plan_backward(P, K, geo, C.c_size_t(-1).value, C.byref(p)) == 0
    return tuple(p[:5])         # accumulation, kernel, row_layout, row_stride, geometry_only
for K in (0, 16, 26, 74):
    assert plan(1000, K, 0) == (0, 3, 0, 16 + 16 * ((K + 5 + 15) // 16), 0), (K, plan(1000, K, 0))
assert plan(1000, 26, 1) == (0, 1, 0, 16, 1), plan(1000, 26, 1)
print("ok")
'''
    from diff_gaussian_rasterization import _abi
    assert C.sizeof(_abi.hsr_backward_plan) == 32 and _abi.hsr_backward_plan.scratch_bytes.offset == 24
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code, _abi.LIB_PATH], cwd=root, env=dict(os.environ, HSR_BWD_IMPL="valu"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
