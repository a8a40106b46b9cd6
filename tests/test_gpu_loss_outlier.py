"""GPU suite for the outlier-rejecting loss head (include/ext/hsr_loss_outlier.h, hsr_utils.losses with ignore_outlier_depth_loss=True).

The oracle of every case is tests/outlier_ref.py (scripts/hierslam.py:909-937 restated in torch) run on the CPU on the same fp32 inputs:
    median, threshold        bit-equal, NaN included
    selected pixels          equal to the reference mask's count
    both terms, the total    within VAL_TOL of tests/test_gpu_losses.py (the bound of hsr_loss_tracking_value) of the float64 sums
    SUM gradients            bit-equal to torch autograd of the restatement (where the depth is NaN torch's abs backward turns the 0 off the
                             mask into 0 * sign(NaN) = NaN; the head writes the 0, as the tracking head does: compared after nan_to_num)
    MEAN gradients           within 1 ulp of torch autograd (the head multiplies by 1 / selected, torch divides by selected)
    gradient off the mask    0
Each case runs in tracking form (C = 3, SUM, silhouette on and off) and in mapping form (C = 0, MEAN), with the upstream gradient 1 and 0.37.
Each case and form also runs through the plain head (hsr_loss_tracking_*, the keyword off) against the restatement without the factor of
:912, under the same bounds: the two heads are one set of kernels (hsr_loss_masked.hip).  A reference sum that is not finite (an infinite
depth on a valid pixel, which only the plain mask selects) must be met by the same non-finite value.
The cases are the smallest shapes at which the selection can go wrong; they are listed at CASES.  The largest distances of the first MI355X
run are in profiles/loss_outlier_gpu.log."""
import functools

import pytest
import torch

import outlier_ref as R
from depth_error_cases import CASES, _DEN, _from_errors, _noisy, _small, _with      # noqa: F401  (the builders and the table live there, shared with the densify select's suite)
from test_gpu_losses import VAL_TOL

pytestmark = pytest.mark.gpu

SIL_THRES = 0.6
NAN, INF = float("nan"), float("inf")


FORMS = ["tracking_sil", "tracking_nosil", "mapping"]
PIXELS_PER_PARTIAL, FINISH_THREADS, OUTLIER_GRID_CAP = 1024, 256, 512


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """the fp32 CPU inputs of a case: depth, gt_depth [H,W]; im, gt_im [3,H,W]; silhouette [H,W]"""
    depth, gt = CASES[case]()
    H, W = depth.shape
    g = torch.Generator().manual_seed(100 + len(case))
    im, gt_im, sil = torch.rand(3, H, W, generator=g), torch.rand(3, H, W, generator=g), torch.rand(H, W, generator=g)
    im[:, 0, 0] = gt_im[:, 0, 0]              # an exact zero of the colour error: gradient 0 there, as torch's sign(0)
    if H * W <= 4:
        sil = torch.ones(H, W)                # the tiny cases are about the median: the silhouette keeps what it selects
    return depth.contiguous(), gt.contiguous(), im, gt_im, sil


@functools.lru_cache(maxsize=None)
def _reference(case, use_sil, reject=True):
    depth, gt, im, gt_im, sil = _inputs(case)
    return R.outlier_ref(depth, gt, im, gt_im, sil if use_sil else None, SIL_THRES, reject)


def _bits(t):
    return t.detach().cpu().reshape(-1).view(torch.int32)


def _same_bits(got, want):
    """bit-equal, where every NaN counts as the same NaN"""
    g, w = got.detach().cpu().reshape(-1), want.detach().cpu().reshape(-1)
    return bool(((_bits(g) == _bits(w)) | (torch.isnan(g) & torch.isnan(w))).all())


def _ulps(a, b):
    """largest distance in units in the last place between two fp32 tensors (ordered-integer view; +0 and -0 coincide)"""
    def ordered(t):
        i = _bits(t).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7fffffff), i)
    return int((ordered(a) - ordered(b)).abs().max())


def _within(got, ref):
    """within VAL_TOL of a finite reference; a reference that is not finite must be met by the same value (NaN by NaN)"""
    if ref != ref or abs(ref) == INF:
        return got == ref or (got != got and ref != ref)
    return abs(got - ref) <= VAL_TOL * abs(ref)


def _raw_value(case, form, scratch=None, reject=True):
    """hsr_loss_outlier_value through the C ABI: (out6, selected) as CPU tensors; reject=False: hsr_loss_tracking_value, (out4, None)"""
    from diff_gaussian_rasterization import _abi
    depth, gt, im, gt_im, sil = (t.cuda() for t in _inputs(case))
    H, W = depth.shape
    tracking, use_sil = form != "mapping", form == "tracking_sil"
    head = "hsr_loss_outlier" if reject else "hsr_loss_tracking"
    out = torch.full((6 if reject else 4,), -7.0, device="cuda")
    sel = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    if scratch is None:
        scratch = torch.empty(int(getattr(_abi.lib, head + "_scratch_bytes")(H, W)), dtype=torch.uint8, device="cuda")
    _abi.call(getattr(_abi.lib, head + "_value"), head + "_value", depth.device, 3 if tracking else 0, H, W,
              im.data_ptr() if tracking else None, gt_im.data_ptr() if tracking else None, depth.data_ptr(), gt.data_ptr(),
              sil.data_ptr() if use_sil else None, SIL_THRES, int(use_sil), 0 if tracking else 1, R.W_DEPTH if tracking else 1.0,
              R.W_IM if tracking else 0.0, out.data_ptr(), *((sel.data_ptr(),) if reject else ()), scratch.data_ptr(), scratch.numel())
    torch.cuda.synchronize()
    return out.cpu(), int(sel.cpu()) if reject else None


def _check_raw(case, form, out6, selected, reject=True):
    """the value pass's outputs against the restatement; returns the largest relative distance of the terms.  reject=False: out6 is the
    plain head's out4, which reports neither median nor count (the count is checked through out4[3] = 1 / count, as for both heads)"""
    ref = _reference(case, form == "tracking_sil", reject)
    if reject:
        assert _same_bits(out6[4], ref["median"]) and _same_bits(out6[5], ref["threshold"]), (case, form, out6[4:], ref["median"], ref["threshold"])
        assert selected == ref["count"], (case, form, selected, ref["count"])
    n = ref["count"]
    if form == "mapping":
        want = [ref["depth_sum"] / n if n else NAN, 0.0]
        want.append(want[0])
    else:
        want = [ref["depth_sum"], ref["colour_sum"], R.W_DEPTH * ref["depth_sum"] + R.W_IM * ref["colour_sum"]]
    worst = 0.0
    for k, w in enumerate(want):
        got = float(out6[k].double())
        if w != w:
            assert got != got, (case, form, k, got)
            continue
        assert _within(got, w), (case, form, k, got, w)
        worst = max(worst, abs(got - w) / abs(w) if w and abs(w) != INF else 0.0)
    inv = float(out6[3])
    assert inv == float(torch.tensor(1.0) / torch.tensor(float(n))) if n else inv == INF
    return worst


@pytest.mark.parametrize("form,reject", [pytest.param(f, r, id=f if r else f + "_plain") for r in (True, False) for f in FORMS])
@pytest.mark.parametrize("case", list(CASES))
def test_value_and_gradients_equal_the_restatement(case, form, reject):
    """reject: the outlier-rejecting head; without it the plain head (the keyword off) against the restatement without the factor of :912"""
    from hsr_utils import losses as L
    depth, gt, im, gt_im, sil = _inputs(case)
    use_sil = form == "tracking_sil"
    ref = _reference(case, use_sil, reject)
    mask = ref["mask"]
    worst = _check_raw(case, form, *_raw_value(case, form, reject=reject), reject=reject)
    median, threshold = L.depth_error_median(depth.cuda(), gt.cuda())
    assert _same_bits(median, ref["median"]) and _same_bits(threshold, ref["threshold"])
    worst_ulps = 0
    for up in (1.0, 0.37):
        d = depth.cuda().reshape(1, *depth.shape).requires_grad_(True)
        if form == "mapping":
            got = L.mapping_depth_loss(d, gt.cuda()[None], ignore_outlier_depth_loss=reject)
            (got * up).backward()
            want_value, want_d = R.autograd_mapping(depth, gt, up, reject)
            g_d = d.grad[0].cpu()
            if ref["count"]:
                assert _within(float(got.detach()), ref["depth_sum"] / ref["count"])
                worst_ulps = max(worst_ulps, _ulps(g_d, torch.nan_to_num(want_d)))
                assert worst_ulps <= 1, (case, up, worst_ulps)
            else:
                assert torch.isnan(got) and torch.isnan(want_value)
        else:
            a = im.cuda().requires_grad_(True)
            res = L.tracking_loss(a, gt_im.cuda(), d, gt.cuda()[None], sil.cuda()[None] if use_sil else None, SIL_THRES, use_sil,
                                  {"depth": R.W_DEPTH, "im": R.W_IM}, return_parts=True, ignore_outlier_depth_loss=reject, return_selected=reject)
            got, parts = res[:2]
            (got * up).backward()
            if reject:      # the plain head returns no count
                count = res[2]
                assert int(count) == ref["count"] and count.dtype == torch.int32 and count.dim() == 0
            assert len(res) == (3 if reject else 2)
            assert _within(float(parts[0]), ref["depth_sum"]) and _within(float(parts[1]), ref["colour_sum"])
            assert _within(float(got.detach()), R.W_DEPTH * ref["depth_sum"] + R.W_IM * ref["colour_sum"])
            want_a, want_d = R.autograd_tracking(depth, gt, im, gt_im, sil if use_sil else None, SIL_THRES, up, reject)
            g_d, g_a = d.grad[0].cpu(), a.grad.cpu()
            assert torch.equal(g_a, want_a) and _ulps(g_a, want_a) == 0, (case, form, up)
            assert torch.equal(g_d, torch.nan_to_num(want_d)) and _ulps(g_d, torch.nan_to_num(want_d)) == 0, (case, form, up)
            assert not g_a[:, ~mask].any()
            if ref["count"] > 1:
                assert g_a[:, mask].any()
        assert not torch.isnan(g_d).any() and not g_d[~mask].any()      # 0 off the mask, whatever the pixel holds
        assert torch.equal(g_d != 0, mask & (depth != gt))                  # on the mask: 0 only at an exact zero of the depth error
    print("loss_outlier %s %s%s: median %.9g selected %d of %d; terms off float64 by %.3g (bound %.1g); mean gradient off torch by %d ulp"
          % (case, form, "" if reject else " (plain head)", float(ref["median"]), ref["count"], mask.numel(), worst, VAL_TOL, worst_ulps))


def test_the_cases_are_what_they_claim():
    """the properties the cases are there for, on the CPU restatement"""
    ref = {c: _reference(c, False) for c in CASES}
    assert ref["1x1_valid"]["count"] == 1 and ref["1x1_hole"]["count"] == 0 and float(ref["1x1_hole"]["median"]) == 0.0
    assert ref["1x2_lower_median"]["count"] == 1 and ref["2x2_lower_median"]["count"] == 2
    assert float(ref["5x7_18_holes"]["median"]) == 0.0 and ref["5x7_18_holes"]["count"] == 0
    assert float(ref["5x7_17_holes"]["median"]) == pytest.approx(0.05) and 0 < ref["5x7_17_holes"]["count"] < 18
    assert ref["equal_errors"]["count"] == int((_inputs("equal_errors")[1] > 0).sum()) > 0
    for c, shift in (("32x32_last_pass", 10), ("32x32_middle_pass", 21)):
        keys = _bits(_inputs(c)[1])
        assert len(set((keys >> shift).tolist())) == 1 and len(set(keys.tolist())) == 1024 and ref[c]["count"] == 1024
    assert len(set((_bits(_inputs("32x32_middle_pass")[1]) & 0x3ff).tolist())) == 1
    assert float(ref["tie_at_threshold"]["threshold"]) == 5.0 and ref["tie_at_threshold"]["count"] == 7
    den = _inputs("denormal_errors")[1]
    assert float(den.max()) < 2.0 ** -126 and float(ref["denormal_errors"]["median"]) == 311000 * _DEN and ref["denormal_errors"]["count"] == 20
    for c in ("nan_depth_valid_pixel", "nan_depth_under_hole", "inf_depth_under_hole"):
        assert torch.isnan(ref[c]["median"]) and ref[c]["count"] == 0
    assert torch.isfinite(ref["inf_depth_valid_pixel"]["median"]) and ref["inf_depth_valid_pixel"]["count"] == 14
    assert ref["negative_gt"]["count"] == 11
    bins = _bits(torch.abs(_inputs("340x600")[1] - _inputs("340x600")[0]) * (_inputs("340x600")[1] > 0))
    m = int(_bits(ref["340x600"]["median"]))
    assert int((bins >> 21 == m >> 21).sum()) > 1000 and int((bins >> 10 == m >> 10).sum()) > 1      # the rank's bin is shared in every pass
    assert 0.8 * 204000 < ref["340x600"]["count"] < 0.97 * 204000
    # the smallest H x W of these aspect ratios past the two limits: one row or column less stays at or under them
    partials = {c: -(-_inputs(c)[0].numel() // PIXELS_PER_PARTIAL) for c in CASES}
    assert 513 * 512 > FINISH_THREADS * PIXELS_PER_PARTIAL >= 512 * 512 and partials["513x512"] == FINISH_THREADS + 1
    assert 725 * 724 > OUTLIER_GRID_CAP * PIXELS_PER_PARTIAL >= 724 * 724 and partials["725x724"] == OUTLIER_GRID_CAP + 1
    assert max(n for c, n in partials.items() if c not in ("513x512", "725x724")) <= FINISH_THREADS      # no other case reaches either
    # the plain mask keeps what the factor of :912 drops: the pixel of infinite depth (its sums are infinite), the 5 % outliers
    plain = {c: _reference(c, False, False) for c in ("inf_depth_valid_pixel", "340x600")}
    assert plain["inf_depth_valid_pixel"]["count"] == 15 and plain["inf_depth_valid_pixel"]["depth_sum"] == INF
    assert plain["340x600"]["count"] > ref["340x600"]["count"] + 0.03 * 204000


def test_scratch_reuse_and_repeat():
    """two calls on ONE scratch with different inputs are each correct, and two calls on the same input give the same bits"""
    from diff_gaussian_rasterization import _abi
    scratch = torch.empty(int(_abi.lib.hsr_loss_outlier_scratch_bytes(129, 67)), dtype=torch.uint8, device="cuda")
    scratch.fill_(0xA5)                       # the head zeroes what it counts into: whatever the scratch held
    first = _raw_value("129x67", "tracking_sil", scratch)
    _check_raw("129x67", "tracking_sil", *first)
    _check_raw("37x23", "mapping", *_raw_value("37x23", "mapping", scratch))
    _check_raw("5x7_18_holes", "tracking_nosil", *_raw_value("5x7_18_holes", "tracking_nosil", scratch))
    again = _raw_value("129x67", "tracking_sil", scratch)
    assert torch.equal(_bits(first[0]), _bits(again[0])) and first[1] == again[1]
    big = (_raw_value("340x600", "tracking_nosil"), _raw_value("340x600", "tracking_nosil"))
    assert torch.equal(_bits(big[0][0]), _bits(big[1][0])) and big[0][1] == big[1][1]


def test_default_path_never_reaches_the_outlier_head(monkeypatch):
    """without the keyword tracking_loss and mapping_depth_loss call what they called before; with it, the new entry point"""
    from diff_gaussian_rasterization import _abi
    from hsr_utils import losses as L
    depth, gt, im, gt_im, sil = (t.cuda() for t in _inputs("37x23"))
    calls = {"outlier": 0, "tracking": 0}
    real_outlier, real_tracking = _abi.lib.hsr_loss_outlier_value, _abi.lib.hsr_loss_tracking_value

    def spy_outlier(*args):
        calls["outlier"] += 1
        return real_outlier(*args)

    def spy_tracking(*args):
        calls["tracking"] += 1
        return real_tracking(*args)
    monkeypatch.setattr(_abi.lib, "hsr_loss_outlier_value", spy_outlier)
    monkeypatch.setattr(_abi.lib, "hsr_loss_tracking_value", spy_tracking)
    plain_t = L.tracking_loss(im, gt_im, depth[None], gt[None], sil[None], SIL_THRES)
    plain_m = L.mapping_depth_loss(depth[None], gt[None])
    off_t = L.tracking_loss(im, gt_im, depth[None], gt[None], sil[None], SIL_THRES, ignore_outlier_depth_loss=False)
    off_m = L.mapping_depth_loss(depth[None], gt[None], ignore_outlier_depth_loss=False)
    assert calls == {"outlier": 0, "tracking": 4}
    assert torch.equal(plain_t, off_t) and torch.equal(plain_m, off_m)
    on_t = L.tracking_loss(im, gt_im, depth[None], gt[None], sil[None], SIL_THRES, ignore_outlier_depth_loss=True)
    on_m = L.mapping_depth_loss(depth[None], gt[None], ignore_outlier_depth_loss=True)
    assert calls == {"outlier": 2, "tracking": 4}
    assert float(on_t) < float(plain_t) and float(on_m) < float(plain_m)      # the outliers are gone from both
