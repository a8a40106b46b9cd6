"""GPU suite for hsr_densify_frame, hsr_prune_mask and hsr_compact_append_rows (include/hsr_densify.h) at their edges, through the C ABI
(diff_gaussian_rasterization._abi) where hsr_utils.densify cannot reach `capacity`, `out_median` or NULL outputs.

The reference of every assertion runs on the CPU on the same fp32 inputs: the reference's expressions in torch (tests/test_densify.torch_reference:
scripts/hierslam.py:1271-1278, :1289-1290) for the median, the threshold and the mask, oracle/densify_oracle.py (held to those expressions by
tests/test_densify_frame_cases_cpu.py) for the emitted rows.  The one comparison between two device results is the one asked for: the select of
hsr_densify_frame (four passes of 8 bits) against hsr_loss_outlier_median (three passes of 11, 11 and 10 bits) on the same two planes.
    median, threshold decisions, mask, count     bit-equal, every NaN counting as the same NaN
    rows                                         row-major pixel order; rgb bit-equal; means, mean_sq_dist and log_scales under the bounds of
                                                 tests/test_gpu_densify.py::test_non_presence_points_match_oracle
The cases are tests/depth_error_cases.py; what each is there for is asserted on the CPU in tests/test_densify_frame_cases_cpu.py.  The output of
the first MI355X run is profiles/densify_frame_edges_gpu.log."""
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
pytestmark = pytest.mark.gpu

SENTINEL, MASK_SENTINEL = -7.0, 0xEE


def _bits(t):
    return t.detach().cpu().reshape(-1).view(torch.int32)


def _same_bits(got, want):
    """bit-equal, where every NaN counts as the same NaN"""
    g, w = got.detach().cpu().reshape(-1), want.detach().cpu().reshape(-1)
    return g.shape == w.shape and bool(((_bits(g) == _bits(w)) | (torch.isnan(g) & torch.isnan(w))).all())


@functools.lru_cache(maxsize=None)
def _case_frame(case):
    return DC.densify_frame(case)


@functools.lru_cache(maxsize=None)
def _case_reference(case):
    return _reference(_case_frame(case))


def _reference(frame, factor=50):
    """the reference's median / threshold / mask (torch) and the oracle's rows, from one c2w"""
    import densify_oracle as DO
    sil, rd, gt, col, K, w2c = frame
    ref = torch_reference(sil, rd, gt, col, K, w2c, DC.SIL_THRES, depth_factor=factor, full=True)
    with np.errstate(all="ignore"):
        o = DO.non_presence_points(sil.numpy(), rd.numpy(), gt.numpy(), col.numpy(), K.numpy(), torch.inverse(w2c).numpy(), DC.SIL_THRES,
                                   depth_factor=factor)
    assert np.array_equal(o["mask"], ref["mask"].numpy())              # the CPU suite's assertion, on this very frame
    return ref, o


def _densify(frame, factor=50.0, capacity=None, rows=None, scratch=None, null=()):
    """hsr_densify_frame through the C ABI.  capacity: H * W unless given; rows: the rows allocated per point output (>= capacity), all
    filled with SENTINEL before the call; null: the outputs passed as NULL.  Returns CPU tensors"""
    from diff_gaussian_rasterization import _abi
    sil, rd, gt, col, K, w2c = frame
    H, W = gt.shape
    N = H * W
    capacity = N if capacity is None else capacity
    rows = max(capacity, 1) if rows is None else rows
    assert rows >= capacity
    dev = torch.device("cuda", torch.cuda.current_device())
    ins = [t.contiguous().to(dev) for t in (sil, rd, gt, col, torch.inverse(w2c))]
    out = {"means": torch.full((rows, 3), SENTINEL, device=dev), "rgb": torch.full((rows, 3), SENTINEL, device=dev),
           "log_scales": torch.full((rows,), SENTINEL, device=dev), "msd": torch.full((rows,), SENTINEL, device=dev),
           "mask": torch.full((N,), MASK_SENTINEL, dtype=torch.uint8, device=dev), "median": torch.full((1,), SENTINEL, device=dev),
           "count": torch.full((1,), -7, dtype=torch.int32, device=dev)}
    p = lambda k: None if k in null else out[k].data_ptr()
    if scratch is None:
        scratch = torch.full((int(_abi.lib.hsr_densify_scratch_bytes(H, W)),), 0xA5, dtype=torch.uint8, device=dev)
    assert scratch.numel() >= int(_abi.lib.hsr_densify_scratch_bytes(H, W))
    _abi.call(_abi.lib.hsr_densify_frame, "hsr_densify_frame", dev, H, W, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(),
              ins[3].data_ptr(), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), ins[4].data_ptr(), DC.SIL_THRES, float(factor),
              capacity, p("count"), p("means"), p("rgb"), p("log_scales"), p("msd"), p("mask"), p("median"), scratch.data_ptr(), scratch.numel())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _loss_head_median(frame):
    """out2[0] of hsr_loss_outlier_median on the frame's rendered and gt depth"""
    from diff_gaussian_rasterization import _abi
    rd, gt = frame[1].cuda(), frame[2].cuda()
    H, W = gt.shape
    out2 = torch.full((2,), SENTINEL, device="cuda")
    scratch = torch.full((int(_abi.lib.hsr_loss_outlier_scratch_bytes(H, W)),), 0xA5, dtype=torch.uint8, device="cuda")
    _abi.call(_abi.lib.hsr_loss_outlier_median, "hsr_loss_outlier_median", rd.device, H, W, rd.data_ptr(), gt.data_ptr(), out2.data_ptr(),
              scratch.data_ptr(), scratch.numel())
    torch.cuda.synchronize()
    return out2.cpu()[0]


def _check(got, ref, o, what, capacity=None):
    """one call's outputs against the references; returns whether the means are bit-equal to the oracle's"""
    mask = ref["mask"]
    M = int(mask.sum())
    assert _same_bits(got["median"], ref["median"]), (what, got["median"], ref["median"])
    assert torch.equal(got["mask"], mask.to(torch.uint8)), (what, (got["mask"] != mask.to(torch.uint8)).nonzero().reshape(-1)[:8])
    assert int(got["count"]) == M, (what, int(got["count"]), M)
    n = M if capacity is None else min(M, capacity)
    assert np.array_equal(got["rgb"][:n].numpy().view(np.uint32), o["rgb"][:n].view(np.uint32)), what      # row-major order, bit for bit
    with np.errstate(all="ignore"):
        np.testing.assert_allclose(got["means"][:n].numpy(), o["means3D"][:n], rtol=1e-6, atol=1e-6, err_msg=what)
        np.testing.assert_allclose(got["msd"][:n].numpy(), o["mean3_sq_dist"][:n], rtol=1e-6, err_msg=what)
        np.testing.assert_allclose(got["log_scales"][:n].numpy(), o["log_scales"][:n], rtol=1e-5, atol=1e-6, err_msg=what)
    for k in ("means", "rgb", "log_scales", "msd"):              # nothing behind the rows that were due
        assert bool((got[k][n:] == SENTINEL).all()), (what, k)
    return np.array_equal(got["means"][:n].numpy().view(np.uint32), o["means3D"][:n].view(np.uint32))


@pytest.mark.parametrize("case", list(DC.ALL_CASES))
def test_median_mask_count_and_rows(case):
    """every case of the table: out_median against torch.median of the CPU error and against the loss head's select; mask, count and rows"""
    frame = _case_frame(case)
    ref, o = _case_reference(case)
    got = _densify(frame)
    other = _loss_head_median(frame)
    print("densify_edges %-26s %4dx%-4d torch median %-14.9g (bits %08x)  densify select %08x  loss-head select %08x  selected %d" % (
        case, frame[2].shape[0], frame[2].shape[1], float(ref["median"]), int(_bits(ref["median"])[0]) & 0xffffffff,
        int(_bits(got["median"])[0]) & 0xffffffff, int(_bits(other)[0]) & 0xffffffff, int(got["count"])))
    assert _same_bits(got["median"], ref["median"]), (case, got["median"], ref["median"])
    assert _same_bits(got["median"], other), (case, got["median"], other)
    exact = _check(got, ref, o, case)
    print("densify_edges %-26s mask, count, order and rgb equal; means bit-equal to the oracle's: %s" % (case, exact))


@pytest.mark.parametrize("factor", [50, 12.5])
@pytest.mark.parametrize("nan_gt", [False, True], ids=["finite", "nan_gt"])
def test_mask_on_its_comparisons(factor, nan_gt):
    """a silhouette at sil_thres and one ulp under it, a NaN silhouette, rendered == gt, an error at depth_factor * median and 2^-11 beyond it,
    gt 0 / negative / NaN, depth_factor 50 and 12.5: the selected pixels are the ones listed at depth_error_cases.comparison_frame"""
    frame, expect = DC.comparison_frame(factor, nan_gt)
    ref, o = _reference(frame, factor)
    assert torch.equal(ref["mask"], expect)
    got = _densify(frame, factor=factor)
    assert got["mask"].nonzero().reshape(-1).tolist() == expect.nonzero().reshape(-1).tolist(), (factor, nan_gt, got["mask"])
    _check(got, ref, o, ("comparisons", factor, nan_gt))
    print("densify_edges comparisons factor %-4s %-6s median %-12.9g selected pixels %s" % (
        factor, "nan_gt" if nan_gt else "finite", float(got["median"]), got["mask"].nonzero().reshape(-1).tolist()))


@pytest.mark.parametrize("which", DC.EMISSION_MASKS)
def test_emission_at_wave_and_block_edges(which):
    """masks set at pixels 63, 64, 255, 256 and N - 1, everywhere, nowhere: the rows are those pixels in row-major order"""
    frame = DC.emission_frame(which)
    ref, o = _reference(frame)
    got = _densify(frame)
    exact = _check(got, ref, o, which)
    M = int(got["count"])
    col = frame[3].permute(1, 2, 0).reshape(-1, 3)
    assert torch.equal(got["rgb"][:M], col[ref["mask"]])            # the colours of exactly those pixels, in that order
    assert M == {"edges": 5, "everywhere": 300, "nowhere": 0}[which]
    print("densify_edges emission %-10s %3d rows in row-major order; means bit-equal to the oracle's: %s" % (which, M, exact))


def test_capacity_truncates_and_count_does_not():
    """capacity 0 with NULL point outputs, 1, M - 1, M, M + 1: out_count is M each time, the first min(M, capacity) rows are the full run's bit
    for bit, every row behind them keeps its sentinel"""
    frame = _case_frame("37x23")
    ref, o = _case_reference("37x23")
    N = frame[2].numel()
    full = _densify(frame)
    M = int(full["count"])
    assert M == int(ref["mask"].sum()) and 2 < M < N
    _check(full, ref, o, "full")
    got = _densify(frame, capacity=0, null=("means", "rgb", "log_scales", "msd"))
    assert int(got["count"]) == M and torch.equal(got["mask"], full["mask"]) and _same_bits(got["median"], full["median"])
    for k in ("means", "rgb", "log_scales", "msd"):
        assert bool((got[k] == SENTINEL).all())
    for capacity in (1, M - 1, M, M + 1):
        got = _densify(frame, capacity=capacity, rows=M + 2)
        n = min(M, capacity)
        assert int(got["count"]) == M and torch.equal(got["mask"], full["mask"]) and _same_bits(got["median"], full["median"]), capacity
        for k in ("means", "rgb", "log_scales", "msd"):
            assert torch.equal(_bits(got[k][:n]), _bits(full[k][:n])), (capacity, k)
            assert bool((got[k][n:] == SENTINEL).all()), (capacity, k)
        _check(got, ref, o, ("capacity", capacity), capacity=capacity)
    print("densify_edges capacity: M = %d of %d pixels; capacities 0, 1, %d, %d, %d leave out_count at M and every row past min(M, capacity) untouched"
          % (M, N, M - 1, M, M + 1))


@pytest.mark.parametrize("absent", ["msd", "mask", "median"])
def test_a_null_output_changes_no_other(absent):
    frame = _case_frame("37x23")
    full = _densify(frame)
    got = _densify(frame, null=(absent,))
    sentinel = MASK_SENTINEL if absent == "mask" else SENTINEL
    assert bool((got[absent] == sentinel).all())
    for k in full:
        if k != absent:
            assert torch.equal(got[k].reshape(-1).view(torch.uint8), full[k].reshape(-1).view(torch.uint8)), (absent, k)


def test_scratch_reuse_and_repeat():
    """a NaN case and then a finite case on ONE scratch that nobody clears: the finite case gives its own result (the NaN count does not
    outlive its call); two calls in a row are bit-equal"""
    from diff_gaussian_rasterization import _abi
    scratch = torch.full((int(_abi.lib.hsr_densify_scratch_bytes(129, 67)),), 0xA5, dtype=torch.uint8, device="cuda")
    for first in ("3x683_nan_last_pixel", "nan_turns_depth_mask_off"):
        got = _densify(_case_frame(first), scratch=scratch)
        assert bool(torch.isnan(got["median"]))
        _check(got, *_case_reference(first), first)
        for second in ("129x67", "3x683", "bucket255_byte0"):
            got = _densify(_case_frame(second), scratch=scratch)
            assert bool(torch.isfinite(got["median"]))
            _check(got, *_case_reference(second), (first, second))
    a, b = _densify(_case_frame("129x67"), scratch=scratch), _densify(_case_frame("129x67"), scratch=scratch)
    for k in a:
        assert torch.equal(a[k].reshape(-1).view(torch.uint8), b[k].reshape(-1).view(torch.uint8)), k
    c = _densify(_case_frame("129x67"))
    for k in a:
        assert torch.equal(a[k].reshape(-1).view(torch.uint8), c[k].reshape(-1).view(torch.uint8)), k


# ---- hsr_prune_mask at its thresholds, and the compaction that follows it -----------------------------------------------------------------
# Inputs on which the decision does not hang on the last bit of an exponential: exp(0) = 1 and exp(-0) = 1 exactly on either side, sigmoid(0) =
# 1 / (1 + 1) = 0.5 exactly, and every other value is far from its threshold (sigmoid(+-90) is 1 and 0 or a denormal; exp(+-1), exp(+-3)).
LOGITS = [0.0, 90.0, -90.0, DC.NAN, 2.0, -2.0, -0.0, 5.0, -0.75]
LOG_SCALES = [0.0, -1.0, 1.0, -0.0, -90.0, 3.0, -3.0]
P_PRUNE = 300                                # two blocks; rows 63, 64, 255, 256 and 299 are set by hand below


def _prune_inputs(S):
    logit = torch.tensor([LOGITS[i % len(LOGITS)] for i in range(P_PRUNE)])
    ls = torch.tensor([[LOG_SCALES[(i * (c + 2) + c) % len(LOG_SCALES)] for c in range(S)] for i in range(P_PRUNE)])
    named = {0: (90.0, 0.0), 1: (-90.0, 0.0), 10: (2.0, 0.0), 11: (2.0, 0.0),
             63: (0.0, 0.0), 64: (-2.0, 0.0), 255: (2.0, 1.0), 256: (DC.NAN, 0.0), 299: (0.0, -1.0)}
    for row, (lo, s) in named.items():
        logit[row], ls[row] = lo, s
    if S == 3:
        ls[255] = torch.tensor([0.0, -1.0, 1.0])          # only the LAST column is over the size threshold
        ls[10] = torch.tensor([1.0, -1.0, 0.0])           # only the first
        ls[11] = torch.tensor([0.0, 0.0, -0.0])           # the maximum is exactly the threshold: kept
        for row, c in ((20, 0), (21, 1), (22, 2)):        # a NaN column beside one over the threshold: torch's maximum is NaN, the row is kept
            logit[row], ls[row] = 2.0, torch.tensor([3.0, 3.0, 0.0])
            ls[row, c] = DC.NAN
    else:
        logit[20], ls[20] = 2.0, DC.NAN                   # NaN > big is false
    return logit.reshape(-1, 1).contiguous(), ls.contiguous()


@pytest.mark.parametrize("S,big", [(1, 1.0), (3, 1.0), (3, 0.0), (1, -1.0)], ids=["S1_big1", "S3_big1", "S3_big0_off", "S1_bigneg_off"])
def test_prune_mask_at_its_thresholds_and_the_rows_it_keeps(S, big):
    """utils/slam_external.py:175-180 with torch CPU ops: to_remove = sigmoid(logit) < 0.5 | max_c exp(log_scale_c) > big (the latter only for
    big > 0).  logit 0 is kept (strict <), +90 kept, -90 removed, NaN kept; log_scale 0 with big = 1 is kept (strict >); S = 3 takes the
    maximum over its columns, which is NaN (and the row kept) as soon as one column is NaN, whichever column; big <= 0 switches the size test
    off.  Then hsr_compact_append_rows on the scanned mask: tensor[keep], then the
    appended rows"""
    from diff_gaussian_rasterization import _abi
    thr = 0.5
    logit, ls = _prune_inputs(S)
    to_remove = (torch.sigmoid(logit) < thr).squeeze(-1)
    if big > 0:
        to_remove = to_remove | (torch.exp(ls).max(dim=1).values > big)
    keep = ~to_remove
    # the named decisions, on the CPU reference itself
    assert keep[63] and not keep[64] and keep[256] and keep[299] and bool(keep[255]) == (big <= 0)      # 0, -2, NaN, 0; log-scale 1 under logit 2
    assert keep[0] and not keep[1]                                                                      # +90, -90
    assert keep[20]                                                                                     # a NaN log-scale
    if S == 3:
        assert bool(keep[11]) and bool(keep[10]) == (big <= 0) and keep[21] and keep[22]
    kept = int(keep.sum())
    assert 0 < kept < P_PRUNE
    dev = torch.device("cuda", torch.cuda.current_device())
    d_logit, d_ls = logit.to(dev), ls.to(dev)
    d_keep = torch.full((P_PRUNE,), MASK_SENTINEL, dtype=torch.uint8, device=dev)
    d_kept = torch.full((1,), -7, dtype=torch.int32, device=dev)
    scratch = torch.full((int(_abi.lib.hsr_compact_scratch_bytes(P_PRUNE)),), 0xA5, dtype=torch.uint8, device=dev)
    _abi.call(_abi.lib.hsr_prune_mask, "hsr_prune_mask", dev, P_PRUNE, S, d_logit.data_ptr(), d_ls.data_ptr(), thr, float(big), d_keep.data_ptr(),
              d_kept.data_ptr(), scratch.data_ptr(), scratch.numel())
    torch.cuda.synchronize()
    assert torch.equal(d_keep.cpu(), keep.to(torch.uint8)), (d_keep.cpu() != keep.to(torch.uint8)).nonzero().reshape(-1)
    assert int(d_kept.cpu()) == kept
    # the rows of a following compaction + append on the same scratch (keep_is_scanned = 1)
    g = torch.Generator().manual_seed(S)
    n_append = 3
    srcs = [torch.rand(P_PRUNE, 3, generator=g), torch.arange(P_PRUNE, dtype=torch.float32).reshape(-1, 1), ls.clone()]
    apps = [torch.rand(n_append, 3, generator=g), None, torch.rand(n_append, S, generator=g)]
    d_src = [t.to(dev) for t in srcs]
    d_app = [t.to(dev) if t is not None else None for t in apps]
    d_dst = [torch.full((P_PRUNE + n_append + 1, t.shape[1]), SENTINEL, device=dev) for t in srcs]
    tabs = (_abi.hsr_row_table * len(srcs))()
    for i in range(len(srcs)):
        tabs[i] = _abi.hsr_row_table(d_src[i].data_ptr(), d_app[i].data_ptr() if d_app[i] is not None else None, d_dst[i].data_ptr(),
                                     int(srcs[i].shape[1]))
    _abi.call(_abi.lib.hsr_compact_append_rows, "hsr_compact_append_rows", dev, P_PRUNE, d_keep.data_ptr(), 1, len(srcs), tabs, n_append,
              d_kept.data_ptr(), scratch.data_ptr(), scratch.numel())
    torch.cuda.synchronize()
    assert int(d_kept.cpu()) == kept + n_append
    for t, a, dst in zip(srcs, apps, d_dst):
        want = torch.cat((t[keep], a if a is not None else torch.zeros(n_append, t.shape[1])))
        got = dst.cpu()
        assert torch.equal(_bits(got[:kept + n_append]), _bits(want)) and bool((got[kept + n_append:] == SENTINEL).all())
    print("densify_edges prune S=%d big=%-4s kept %d of %d rows; keep mask, count and compacted rows equal tensor[keep]" % (S, big, kept, P_PRUNE))
