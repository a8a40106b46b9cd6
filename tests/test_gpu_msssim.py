"""GPU suite for the multi-scale SSIM (include/ext/hsr_msssim.h, hsr_utils.evaluate.ms_ssim): the score and every per-scale,
per-channel mean against the float64 restatement of tests/msssim_ref.py (which its scipy sibling confirms to 1e-12 in
tests/test_msssim_cpu.py), bit-repeatability, the evaluate_frame flag, and the refusals.

The bound is the project's for float outputs, 1e-4, absolute: every quantity lies in [-1, 1].  An fp32 restatement of the same steps
(msssim_torch in float32, on the host) is the yardstick for what fp32 arithmetic costs; each case prints the kernel's and that
restatement's distances from float64 side by side.

Measured on an MI355X (profiles/msssim_gpu_suite.log), the largest over the cases of this file: kernel 2.5e-5 on a per-scale mean
(176x193 noise, last scale: a 1x3-pixel map) and 1.0e-6 on the score; the fp32 restatement 2.4e-5 (161x161 noise, last scale: one
pixel) and 1.3e-6.  At 680x1200: kernel 1.9e-7 / 5.1e-8, restatement 1.5e-7 / 1.2e-7.  On no case is the kernel's distance above 1e-5
and more than four times the restatement's (the widest ratio is 2.2 at 176x193 noise, 2.5e-5 against 1.1e-5: two fp32 evaluations
of a cancelling variance that sum their taps in different orders, averaged over three pixels); each case asserts that criterion, for
the table and for the score.  tests/test_gpu_msssim_tiles.py looks below these means: the pyramid bit for bit and every tile's sums.
"""
import numpy as np
import pytest
import torch

import msssim_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-4
CASES = R.cases()


def _ev():
    from hsr_utils import evaluate as E
    return E


def _device_args(case):
    im, gt, depth, opacity, thres = R.reference(case)[:5]
    args = [im.cuda(), gt.cuda(), depth.cuda()]
    return args + ([opacity.cuda(), thres] if case[4] else [None, None])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_matches_float64_restatement_and_repeats(case):
    E = _ev()
    im, gt, depth, opacity, thres, score64, table64 = R.reference(case)
    args = _device_args(case)
    score, table = E.ms_ssim(*args, details=True)
    again = E.ms_ssim(*args, details=True)
    assert score.is_cuda and score.dim() == 0 and score.dtype == torch.float64 and table.shape == (5, 3, 2)
    d_score, d_table = abs(score.item() - score64), np.abs(table.cpu().numpy() - table64)
    score32, table32 = R.msssim_torch(*R.masked(im, gt, depth, opacity if case[4] else None, thres), torch.float32)
    f_score, f_table = abs(score32 - score64), np.abs(table32 - table64)
    print("\n%s: ms_ssim %.6f | kernel - f64: score %.2e, per-scale mean %.2e (scale %d) | fp32 restatement - f64: score %.2e, "
          "per-scale mean %.2e (scale %d)" % (case[0], score64, d_score, d_table.max(), d_table.max((1, 2)).argmax(), f_score,
                                              f_table.max(), f_table.max((1, 2)).argmax()))
    assert d_score <= TOL, (score.item(), score64)
    assert d_table.max() <= TOL, d_table.max((1, 2))
    # the docstring's criterion: never above 1e-5 AND more than four times what the fp32 restatement costs
    assert not (d_table.max() > 1e-5 and d_table.max() > 4 * f_table.max()), (d_table.max(), f_table.max())
    assert not (d_score > 1e-5 and d_score > 4 * f_score), (d_score, f_score)
    assert torch.equal(score, again[0]) and torch.equal(table, again[1])
    assert torch.equal(E.ms_ssim(*args), score)


def test_depth_plane_with_leading_axis_and_masks_match_explicit_masking():
    """[1,H,W] planes are taken like [H,W]; masking inside the kernel equals masking the images first, bit for bit"""
    E = _ev()
    case = next(c for c in CASES if c[0] == "161x178-masked-sil")
    im, gt, depth, opacity, thres = (t.cuda() if isinstance(t, torch.Tensor) else t for t in R.reference(case)[:5])
    a = E.ms_ssim(im, gt, depth[None], opacity[None], thres, details=True)
    x, y = R.masked(im, gt, depth, opacity, thres)
    b = E.ms_ssim(x, y, torch.ones_like(depth), details=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_evaluate_frame_flag():
    E = _ev()
    case = next(c for c in CASES if c[0] == "176x193-texture-sil")
    im, gt, gt_d, opacity, thres = _device_args(case)
    H, W = gt_d.shape
    g = torch.Generator().manual_seed(5)
    depth = (gt_d.cpu() + 0.1 * torch.randn(H, W, generator=g)).cuda()
    sem = torch.randn(4, H, W, generator=g).cuda()
    gt_lab = torch.randint(0, 4, (H, W), generator=g).cuda()
    kw = dict(final_opacity=opacity, sil_thres=thres, num_classes=4)
    plain = E.evaluate_frame(im, gt, depth, gt_d, sem, gt_lab, "flat", **kw)
    assert list(plain) == ["psnr", "depth_l1", "depth_rmse", "miou", "mbiou"]
    flagged = E.evaluate_frame(im, gt, depth, gt_d, sem, gt_lab, "flat", ms_ssim=True, **kw)
    assert list(flagged) == list(plain) + ["ms_ssim"]
    assert all(torch.equal(flagged[k], plain[k]) for k in plain)
    v = flagged["ms_ssim"]
    assert v.is_cuda and v.dim() == 0 and torch.equal(v, E.ms_ssim(im, gt, gt_d, opacity, thres))
    assert abs(v.item() - R.reference(case)[5]) <= TOL


def test_illegal_sizes_and_cpu_tensors_raise():
    E = _ev()
    for H, W in ((160, 300), (300, 160), (64, 64)):
        x = torch.rand(3, H, W, device="cuda")
        with pytest.raises(AssertionError, match="larger than 160"):
            E.ms_ssim(x, x, x[0])
    x = torch.rand(3, 161, 161, device="cuda")
    assert E.ms_ssim(x, x, torch.ones_like(x[0])).item() == 1.0
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.ms_ssim(x.cpu(), x, x[0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.ms_ssim(x, x, x[0].cpu())
    with pytest.raises(RuntimeError, match="go together"):
        E.ms_ssim(x, x, x[0], final_opacity=x[0])
    with pytest.raises(RuntimeError, match="differs from im"):
        E.ms_ssim(x, x[:, :, :160], x[0])
    with pytest.raises(RuntimeError, match=r"must be \[3,H,W\]"):
        E.ms_ssim(x[:2], x[:2], x[0])
    # the library's own refusals, below the Python checks
    lib = E._lib
    out = torch.zeros(31, dtype=torch.float64, device="cuda")
    assert lib.hsr_eval_msssim(160, 161, x.data_ptr(), x.data_ptr(), x.data_ptr(), None, 0.0, out.data_ptr(), None, 0, None) == -1
    assert lib.hsr_eval_msssim(161, 161, x.data_ptr(), x.data_ptr(), x.data_ptr(), None, 0.0, out.data_ptr(), out.data_ptr(), 8, None) == -2
    assert b"scratch" in lib.hsr_last_error()
