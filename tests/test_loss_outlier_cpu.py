"""CPU suite for the outlier-rejecting loss head (include/ext/hsr_loss_outlier.h): the names of its prototypes and of its table in
_abi.py (tests/test_abi.py checks that they are exported and bound with the header's types), the argument checks that precede any
launch, and the torch restatement tests/outlier_ref.py (rank rule, NaN).  Nothing here launches: there is no GPU."""
import pytest
import torch

import outlier_ref as R
import test_abi

EXT_HEADER = "ext/hsr_loss_outlier.h"
NAMES = ["hsr_loss_outlier_scratch_bytes", "hsr_loss_outlier_median", "hsr_loss_outlier_value", "hsr_loss_outlier_grad"]


def test_loss_outlier_abi_exported_and_bound():
    from diff_gaussian_rasterization import _abi
    protos = test_abi._prototypes([EXT_HEADER])
    assert [s[0] for s in _abi.HEADERS[EXT_HEADER]] == list(protos) == NAMES      # the header's order


def test_loss_outlier_refuses_before_any_device_work():
    """an error code and a message, not a launch: every pointer here is NULL or a made-up address that nothing reads on the host"""
    from diff_gaussian_rasterization import _abi
    lib = _abi.lib
    null, p = None, 1 << 20      # p: a non-NULL, 16-byte aligned value for pointer parameters
    need = lib.hsr_loss_outlier_scratch_bytes(680, 1200)
    assert 3 * 2048 * 4 <= need < 64 * 1024 and lib.hsr_loss_outlier_scratch_bytes(1, 1) == need      # three histograms; no H * W term

    def value(Cc=3, H=8, W=8, im=p, gt_im=p, depth=p, gt=p, sil=p, use_sil=1, reduction=0, out6=p, sel=p, scratch=p, nbytes=need):
        return lib.hsr_loss_outlier_value(Cc, H, W, im, gt_im, depth, gt, sil, 0.5, use_sil, reduction, 1.0, 0.5, out6, sel, scratch, nbytes, null)

    def grad(Cc=3, H=8, W=8, im=p, gt_im=p, depth=p, gt=p, sil=p, use_sil=1, thr=p):
        return lib.hsr_loss_outlier_grad(Cc, H, W, im, gt_im, depth, gt, sil, 0.5, use_sil, 1.0, 0.5, thr, null, null, p, p, null)

    def median(H=8, W=8, depth=p, gt=p, out2=p, scratch=p, nbytes=need):
        return lib.hsr_loss_outlier_median(H, W, depth, gt, out2, scratch, nbytes, null)

    for kw in (dict(H=0), dict(W=0), dict(H=-3), dict(H=65536, W=32768), dict(depth=null), dict(gt=null)):
        for fn, who in ((value, b"loss_outlier_value"), (grad, b"loss_outlier_grad"), (median, b"loss_outlier_median")):
            assert fn(**kw) == -1 and who in lib.hsr_last_error(), (kw, who)
    for kw in (dict(Cc=1), dict(Cc=4), dict(Cc=-1), dict(im=null), dict(gt_im=null), dict(sil=null)):
        for fn, who in ((value, b"loss_outlier_value"), (grad, b"loss_outlier_grad")):
            assert fn(**kw) == -1 and who in lib.hsr_last_error() and b"C=" in lib.hsr_last_error(), (kw, who)
    for kw in (dict(reduction=2), dict(reduction=-1), dict(out6=null), dict(sel=null)):
        assert value(**kw) == -1 and b"reduction" in lib.hsr_last_error(), kw
    assert median(out2=null) == -1 and b"out2" in lib.hsr_last_error()
    assert grad(thr=null) == -1 and b"threshold" in lib.hsr_last_error()
    for fn in (value, median):
        for kw in (dict(nbytes=need - 1), dict(nbytes=0), dict(scratch=null), dict(scratch=p + 4)):
            assert fn(**kw) == _abi.HSR_ERR_BUFFER_TOO_SMALL and b"scratch" in lib.hsr_last_error(), kw
    # C = 0 needs no image and no silhouette pointer: the arguments pass, and with both outputs NULL the gradient has nothing to launch
    assert lib.hsr_loss_outlier_grad(0, 8, 8, null, null, p, p, null, 0.5, 0, 1.0, 0.0, p, null, null, null, null, null) == 0


def test_cpu_tensors_are_refused():
    from hsr_utils import losses as L
    z, d = torch.zeros(3, 8, 8), torch.ones(1, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        L.tracking_loss(z, z, d, d, d, ignore_outlier_depth_loss=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        L.mapping_depth_loss(d, d, ignore_outlier_depth_loss=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        L.depth_error_median(d, d)
    with pytest.raises(RuntimeError, match="ignore_outlier_depth_loss"):
        L.tracking_loss(z, z, d, d, d, return_selected=True)


@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_rank_rule_is_torch_median(n):
    """the header's rank rule, sort()[(n - 1) // 2], is what torch.median returns and what the restatement's threshold is built on"""
    g = torch.Generator().manual_seed(n)
    v = torch.rand(n, generator=g)
    want = v.sort().values[(n - 1) // 2]
    assert torch.equal(R.rank_rule(v), want) and torch.equal(v.median(), want)
    gt = v + 1.0                                  # errors gt - 0 = gt, all valid
    median, threshold, mask = R.outlier_mask(torch.zeros(1, n), gt.reshape(1, n))
    assert torch.equal(median, gt.sort().values[(n - 1) // 2]) and torch.equal(threshold, 10 * median) and bool(mask.all())
    if n % 2 == 0:                                # the LOWER of the two middle values
        assert float(median) < float(gt.sort().values[n // 2])


def test_lower_median_decides_a_mask():
    """errors {1, 20}: the lower median 1 gives the threshold 10 and selects one pixel; an upper median would select both"""
    ref = R.outlier_ref(torch.zeros(1, 2), torch.tensor([[1.0, 20.0]]))
    assert float(ref["median"]) == 1.0 and float(ref["threshold"]) == 10.0 and ref["mask"].tolist() == [[True, False]]
    assert ref["count"] == 1 and ref["depth_sum"] == 1.0


def test_a_nan_error_empties_the_mask():
    gt = torch.tensor([[1.0, 2.0, 0.0, 4.0, 5.0]])
    for depth in (torch.tensor([[0.5, float("nan"), 1.0, 3.0, 4.0]]),            # a NaN depth on a valid pixel
                  torch.tensor([[0.5, 1.0, float("nan"), 3.0, 4.0]]),            # a NaN depth under a hole: still a NaN error
                  torch.tensor([[0.5, 1.0, float("inf"), 3.0, 4.0]])):           # inf * 0 is NaN
        ref = R.outlier_ref(depth, gt)
        assert torch.isnan(ref["median"]) and torch.isnan(ref["threshold"]) and torch.isnan(R.rank_rule(torch.abs(gt - depth) * (gt > 0)))
        assert ref["count"] == 0 and not ref["mask"].any() and ref["depth_sum"] == 0.0
        mean, grad = R.autograd_mapping(depth, gt, 1.0)
        assert torch.isnan(mean) and not torch.nan_to_num(grad).any()
    ref = R.outlier_ref(torch.tensor([[0.5, 1.0, 1.0, float("inf"), 4.0]]), gt)   # inf on a valid pixel: the median stays finite
    assert float(ref["median"]) == 1.0 and ref["mask"].tolist() == [[True, True, False, False, True]]
