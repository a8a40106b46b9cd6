"""Fused loss heads (hier-slam_amd/csrc/hsr_losses.hip) at the dispatch cells, thresholds and inputs that tests/test_gpu_losses.py
leaves unrun, every comparison against oracle/loss_oracle.py (numpy float64):

  leaf head   all nine leaf_mlp_ce_kernel<KU, MAXCT> instances and the six edges of that choice, K = 1, C = 1, one class tile / two;
              a second trip of the persistent loop; NULL gradient outputs through the C ABI; logits of +-60
  tree CE     16 / 17 channels (registers / streamed), one-class levels, 16 levels, the add_grad join on every path and on the spare
              channels, the finish kernel's four-loads-in-flight branch, logits of +-80
  labels      out of range on every path: "matching no class" (include/hsr_losses.h)
  SSIM        sizes that are a multiple of the 32 x 32 tile, one past it, one pixel, and a zero-variance image

Which instance a (K, C) pair of the leaf head runs (hsr_loss_leaf_mlp_ce: KU = K + 1 rounded up to 4, then the next of 20 / 28 / 32;
MAXCT = class tiles of 16, then the next of 3 / 7 / 8).  Edges: K 19|20 and 27|28, C 48|49 and 112|113; C 16|17 is one tile | two.

      K \\ C       1, 16, 17, 48      49, 112      113, 128
      1, 3, 19     (20, 3)            (20, 7)      (20, 8)
      20, 27       (28, 3)            (28, 7)      (28, 8)
      28, 31       (32, 3)            (32, 7)      (32, 8)
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
pytestmark = pytest.mark.gpu

# the bounds of tests/test_gpu_losses.py, as they stand there
SSIM_VAL_TOL = 1e-5
SSIM_GRAD_TOL = 5e-4
GRAD_TOL = 2e-6
LEVEL_RTOL = 3e-6          # per-level tree losses against the oracle
LEAF_LOSS_TOL = 5e-6       # x max(1, |loss|)
LEAF_DSEM_TOL = 1e-5       # of the largest entry
LEAF_DW_TOL = 2e-5         # d_weight, d_bias, of the largest entry


def _relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _np(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------- leaf head
def _leaf_data(K, Cc, H, W, seed, wscale=1.0):
    """random data as test_leaf_mlp_head_against_oracle draws them, a few ignored labels"""
    g = np.random.default_rng(seed)
    sem = g.normal(0, 1.5, (K, H, W)).astype(np.float32)
    w, b = (wscale * g.normal(0, 0.4, (Cc, K))).astype(np.float32), g.normal(0, 0.3, (Cc,)).astype(np.float32)
    lab = g.integers(0, Cc, (H, W)).astype(np.int64)
    lab[0, :5] = -100
    return sem, w, b, lab


def _leaf_fused(sem, w, b, lab, up):
    from hsr_utils import losses as L
    Cc, K = w.shape
    ts = torch.tensor(sem, device="cuda", requires_grad=True)
    tw = torch.tensor(w.reshape(Cc, K, 1, 1), device="cuda", requires_grad=True)
    tb = torch.tensor(b, device="cuda", requires_grad=True)
    loss = L.leaf_mlp_cross_entropy(ts, (tw, tb), torch.tensor(lab, device="cuda"))
    (up * loss).backward()
    return loss.detach(), ts.grad, tw.grad.reshape(Cc, K), tb.grad


def _leaf_eager(sem, w, b, lab, up):
    """the torch chain the head replaces, fp32 on the device: conv2d + F.cross_entropy"""
    Cc, K = w.shape
    ts = torch.tensor(sem, device="cuda", requires_grad=True)
    tw = torch.tensor(w.reshape(Cc, K, 1, 1), device="cuda", requires_grad=True)
    tb = torch.tensor(b, device="cuda", requires_grad=True)
    z = torch.nn.functional.conv2d(ts.unsqueeze(0), tw, tb)[0]
    loss = torch.nn.functional.cross_entropy(z.reshape(Cc, -1).t(), torch.tensor(lab, device="cuda").reshape(-1))
    (up * loss).backward()
    return loss.detach(), ts.grad, tw.grad.reshape(Cc, K), tb.grad


def _leaf_distances(got, ref, up):
    lo, ds, dw, db = ref
    return (abs(float(got[0]) - lo), _relmax(_np(got[1]), up * ds), _relmax(_np(got[2]), up * dw), _relmax(_np(got[3]), up * db))


@pytest.mark.parametrize("Cc", [1, 16, 17, 48, 49, 112, 113, 128])
@pytest.mark.parametrize("K", [1, 3, 19, 20, 27, 28, 31])
def test_leaf_head_every_instance_and_dispatch_edge(K, Cc):
    """23 x 29 = 667 pixels: two full workgroups, then one that ends in a partial wave"""
    import loss_oracle as LO
    H, W, up = 23, 29, 1.75
    sem, w, b, lab = _leaf_data(K, Cc, H, W, 1000 * K + Cc)
    loss, d_sem, d_w, d_b = _leaf_fused(sem, w, b, lab, up)
    lo, ds, dw, db = LO.leaf_mlp_cross_entropy(sem, w, b, lab)
    if Cc == 1:
        # one class: log-sum-exp = the logit, softmax = 1
        print("K=%d C=1: loss %.3e, max |d_sem| %.3e |d_w| %.3e |d_b| %.3e" % (K, float(loss), float(d_sem.abs().max()), float(d_w.abs().max()),
                                                                           float(d_b.abs().max())))
        assert lo == 0.0 and float(loss) == 0.0
        for got, want in ((d_sem, ds), (d_w, dw), (d_b, db)):
            assert np.abs(_np(got) - up * want).max() <= 1e-7
        return
    e = _leaf_distances((loss, d_sem, d_w, d_b), (lo, ds, dw, db), up)
    print("K=%d C=%d: loss %.3e  d_sem %.3e  d_weight %.3e  d_bias %.3e" % ((K, Cc) + e))
    assert e[0] < LEAF_LOSS_TOL * max(1.0, abs(lo))
    assert e[1] < LEAF_DSEM_TOL
    assert e[2] < LEAF_DW_TOL and e[3] < LEAF_DW_TOL


# d_weight / d_bias of the two cases below sum 307 200 and 250 000 fp32 terms, 2 to 3 times the 150 000 that set LEAF_DW_TOL.  The bound is
# the larger of LEAF_DW_TOL and twice the distance of torch's own fp32 chain (conv2d + F.cross_entropy on the device) from the float64
# oracle, measured in the test and printed by it.  The same chain in fp32 on the CPU (of the largest entry; no device figure has been taken
# yet, the test prints both):
#                               eager d_weight  d_bias
#   K =  3, C =   5, 512 x 600  8.4e-08         9.1e-06      (d_bias nearly cancels: its largest entry is small)
@pytest.mark.parametrize("K,Cc,H,W", [(3, 5, 512, 600), (26, 102, 500, 500)])
def test_leaf_head_second_trip_of_the_persistent_loop(K, Cc, H, W):
    """more than 768 x 256 pixels: 1 200 (977) blocks of work on 768 workgroups, so 432 (209) of them go round the pixel loop twice and
    carry s_st, the panel and the MFMA accumulators into the second trip"""
    import loss_oracle as LO
    assert H * W > 768 * 256
    up = 1.75
    sem, w, b, lab = _leaf_data(K, Cc, H, W, K * Cc)
    got = _leaf_fused(sem, w, b, lab, up)
    ref = LO.leaf_mlp_cross_entropy(sem, w, b, lab)
    e = _leaf_distances(got, ref, up)
    q = _leaf_distances(_leaf_eager(sem, w, b, lab, up), ref, up)
    print("K=%d C=%d %dx%d fused: loss %.3e d_sem %.3e d_weight %.3e d_bias %.3e | eager: loss %.3e d_sem %.3e d_weight %.3e d_bias %.3e"
          % ((K, Cc, H, W) + e + q))
    assert e[0] < LEAF_LOSS_TOL * max(1.0, abs(ref[0]))
    assert e[1] < LEAF_DSEM_TOL
    assert e[2] < max(LEAF_DW_TOL, 2 * q[2]) and e[3] < max(LEAF_DW_TOL, 2 * q[3])
    again = _leaf_fused(sem, w, b, lab, up)
    for x, y in zip(got, again):
        assert torch.equal(x, y)                                    # fixed partition, fixed-order finish


def test_leaf_head_null_outputs_through_the_c_abi():
    """d_sem, d_weight, d_bias may each be NULL: the loss and whatever is asked for do not depend on what else is"""
    from hsr_utils import losses as L
    K, Cc, H, W = 16, 41, 23, 29
    sem, w, b, lab = _leaf_data(K, Cc, H, W, 7)
    ts, tw, tb, tl = (torch.tensor(a, device="cuda") for a in (sem, w, b, lab))
    sc = torch.empty(int(L._lib.hsr_loss_scratch_bytes(K, H, W)), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(want_sem, want_wb):
        out = torch.full((1,), float("nan"), device="cuda")
        d_sem = torch.full_like(ts, float("nan")) if want_sem else None
        d_w = torch.full_like(tw, float("nan")) if want_wb else None
        d_b = torch.full_like(tb, float("nan")) if want_wb else None
        sc.fill_(0xff)
        rc = L._lib.hsr_loss_leaf_mlp_ce(K, Cc, H, W, ts.data_ptr(), tw.data_ptr(), tb.data_ptr(), tl.data_ptr(), -100, out.data_ptr(),
                                         None if d_sem is None else d_sem.data_ptr(), None if d_w is None else d_w.data_ptr(),
                                         None if d_b is None else d_b.data_ptr(), sc.data_ptr(), sc.numel(), s)
        assert rc == 0
        torch.cuda.synchronize()
        return out, d_sem, d_w, d_b
    full = call(True, True)
    assert all(bool(torch.isfinite(x).all()) for x in full)
    for want_sem, want_wb in ((False, True), (True, False), (False, False)):
        got = call(want_sem, want_wb)
        for x, y in zip(full, got):
            assert y is None or torch.equal(x, y), (want_sem, want_wb)


# ---------------------------------------------------------------- tree cross-entropy
def _tree_labels(g, sizes, H, W):
    lab = np.stack([g.integers(0, n, (H, W)) for n in sizes]).astype(np.int64)
    lab[0, :2] = -100
    lab[-1, 3, 4:9] = -100
    return lab


def _tree_both_forms(z, lab, sizes, w, up):
    """(levels, gradient) of the autograd form (hsr_loss_tree_ce_value / _grad) with weights and an upstream gradient, and of the one-call
    hsr_loss_tree_ce with the same weights"""
    from hsr_utils import losses as L
    K, H, W = z.shape
    n = len(sizes)
    tz = torch.tensor(z, device="cuda", requires_grad=True)
    tl = torch.tensor(lab, device="cuda")
    total, levels = L.tree_cross_entropy(tz, tl, sizes, weights=w, return_levels=True)
    (up * total).backward()
    csz, cw = (C.c_int * n)(*sizes), (C.c_float * n)(*w)
    out1, grad1 = torch.empty(n, device="cuda"), torch.full_like(tz, float("nan"))
    sc = torch.empty(int(L._lib.hsr_loss_scratch_bytes(K, H, W)), dtype=torch.uint8, device="cuda")
    assert L._lib.hsr_loss_tree_ce(K, H, W, n, csz, cw, tz.data_ptr(), tl.data_ptr(), -100, out1.data_ptr(), grad1.data_ptr(), sc.data_ptr(),
                                   sc.numel(), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    return (_np(levels), _np(tz.grad)), (_np(out1), _np(grad1)), float(total)


def _weighted(go, sizes, w, K):
    gw, b = go.copy(), 0
    for n, wl in zip(sizes, w):
        gw[b:b + n] *= np.float32(wl)
        b += n
    assert not gw[b:K].any()
    return gw


def _check_tree(z, lab, sizes, tag):
    """both forms against the oracle (LEVEL_RTOL, GRAD_TOL) and against each other (level losses bit for bit, gradients at GRAD_TOL)"""
    import loss_oracle as LO
    K = z.shape[0]
    w = [0.5 + 0.25 * (i % 7) for i in range(len(sizes))]
    up = 3.5
    (lv2, g2), (lv1, g1), total = _tree_both_forms(z, lab, sizes, w, up)
    lo, go = LO.tree_cross_entropy(z, lab, sizes)
    gw = _weighted(go, sizes, w, K)
    den = np.where(lo == 0, 1.0, np.abs(lo))
    print("%s: levels two-pass %.2e one-pass %.2e (relative); grad two-pass %.2e one-pass %.2e" % (
        tag, (np.abs(lv2 - lo) / den).max(), (np.abs(lv1 - lo) / den).max(), _relmax(g2, up * gw), _relmax(g1, gw)))
    assert np.isfinite(lv1).all() and np.isfinite(lv2).all() and np.isfinite(g1).all() and np.isfinite(g2).all()
    np.testing.assert_allclose(lv2, lo, rtol=LEVEL_RTOL)
    np.testing.assert_allclose(lv1, lo, rtol=LEVEL_RTOL)
    assert abs(total - float(np.dot(w, lo))) <= 1e-5 * max(1.0, abs(float(np.dot(w, lo))))
    assert _relmax(g2, up * gw) < GRAD_TOL and _relmax(g1, gw) < GRAD_TOL
    assert np.array_equal(lv2, lv1)                                 # the one-call entry runs the same two passes
    assert _relmax(g2, up * g1) < GRAD_TOL
    b = 0
    for l, n in enumerate(sizes):
        if n == 1:                                                  # a one-class level: loss 0 and gradient 0 exactly
            assert lv1[l] == 0 and lv2[l] == 0 and not g1[b].any() and not g2[b].any()
        b += n
    assert not g1[b:].any() and not g2[b:].any()                    # channels behind the last level
    return lo, go


TREE_LAYOUTS = [([16], 16), ([17], 17), ([1], 1), ([1, 16, 17, 2], 38), (list(range(1, 17)), 136)]


@pytest.mark.parametrize("sizes,K", TREE_LAYOUTS, ids=["16", "17", "1", "1_16_17_2_spare2", "sixteen_levels"])
def test_tree_ce_register_stream_edge_and_degenerate_levels(sizes, K):
    """CE_REG = 16 channels stay in registers, 17 stream; one-class levels; HSR_LOSS_MAX_LEVELS levels; two spare channels"""
    H, W = 19, 33
    g = np.random.default_rng(K)
    z = g.normal(0, 3, (K, H, W)).astype(np.float32)
    _check_tree(z, _tree_labels(g, sizes, H, W), sizes, "layout %s" % sizes)


@pytest.mark.parametrize("with_scale", [True, False], ids=["device_scale", "null_scale"])
def test_tree_ce_grad_joins_another_heads_gradient_on_every_path(with_scale):
    """hsr_loss_tree_ce_grad with add_grad: out = tree part + add_grad * add_scale[0] * add_host_scale on a one-class level, a register
    level, a streamed level, and on the two spare channels behind the last level, where the tree part is 0"""
    import loss_oracle as LO
    from hsr_utils import losses as L
    sizes, K, H, W = [1, 16, 17, 2], 38, 19, 33
    n = len(sizes)
    g = np.random.default_rng(38)
    z = g.normal(0, 3, (K, H, W)).astype(np.float32)
    lab = _tree_labels(g, sizes, H, W)
    add = g.normal(0, 1e-3, (K, H, W)).astype(np.float32)           # the size of a mean-reduced gradient at this map
    w, up, a_dev, a_host = [1.0, 0.25, 2.0, 1.5], np.float32(3.5), np.float32(1.3), 0.5
    tz, tl, ta = (torch.tensor(a, device="cuda") for a in (z, lab, add))
    t_up, t_as = torch.tensor([up], device="cuda"), torch.tensor([a_dev], device="cuda")
    csz, cw = (C.c_int * n)(*sizes), (C.c_float * n)(*w)
    lv, inv = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    sc = torch.empty(int(L._lib.hsr_loss_tree_ce_scratch_bytes(H, W)), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert L._lib.hsr_loss_tree_ce_value(K, H, W, n, csz, tz.data_ptr(), tl.data_ptr(), -100, lv.data_ptr(), inv.data_ptr(), sc.data_ptr(),
                                         sc.numel(), s) == 0
    out = torch.full_like(tz, float("nan"))
    assert L._lib.hsr_loss_tree_ce_grad(K, H, W, n, csz, cw, tz.data_ptr(), tl.data_ptr(), -100, inv.data_ptr(), t_up.data_ptr(), ta.data_ptr(),
                                        t_as.data_ptr() if with_scale else None, a_host, out.data_ptr(), s) == 0
    torch.cuda.synchronize()
    lo, go = LO.tree_cross_entropy(z, lab, sizes)
    scale = (float(a_dev) if with_scale else 1.0) * a_host
    want = _weighted(go, sizes, w, K) * float(up) + add.astype(np.float64) * scale
    got = _np(out)
    print("join (%s): %.2e of the largest entry; spare channels %.2e" % ("scale" if with_scale else "NULL scale", _relmax(got, want),
                                                                        _relmax(got[36:], want[36:])))
    assert np.isfinite(got).all()
    assert _relmax(got, want) < GRAD_TOL
    assert np.abs(want[36:]).max() > 0 and _relmax(got[36:], want[36:]) < GRAD_TOL       # the spare channels hold the other head's part alone
    assert _relmax(got[0:1], want[0:1]) < GRAD_TOL                                       # as does the one-class level


def test_tree_ce_finish_kernel_with_four_loads_in_flight():
    """330 x 320 = 105 600 pixels = 104 value-pass blocks of 1 024: above the 96 at which tree_ce_finish_kernel unrolls by four.  Level 2 has
    fewer valid pixels than the others, so a count taken from the wrong column shows."""
    import loss_oracle as LO
    from hsr_utils import losses as L
    sizes, K, H, W = [2, 4, 6, 6, 8], 26, 330, 320
    assert (H * W + 1023) // 1024 > 96
    g = np.random.default_rng(330)
    z = g.normal(0, 3, (K, H, W)).astype(np.float32)
    lab = np.stack([g.integers(0, n, (H, W)) for n in sizes]).astype(np.int64)
    lab[2, 100:107] = -100
    lab[2, 329, 300:] = -100
    w, up = [1.0, 0.25, 2.0, 1.5, 0.5], 3.5
    tz = torch.tensor(z, device="cuda", requires_grad=True)
    total, levels = L.tree_cross_entropy(tz, torch.tensor(lab, device="cuda"), sizes, weights=w, return_levels=True)
    (up * total).backward()
    lo, go = LO.tree_cross_entropy(z, lab, sizes)
    print("finish: levels %s grad %.2e" % (np.abs(_np(levels) / lo - 1), _relmax(_np(tz.grad), up * _weighted(go, sizes, w, K))))
    np.testing.assert_allclose(_np(levels), lo, rtol=LEVEL_RTOL)
    assert _relmax(_np(tz.grad), up * _weighted(go, sizes, w, K)) < GRAD_TOL


# ---------------------------------------------------------------- out-of-range labels
def test_out_of_range_labels_match_no_class_on_every_tree_path():
    """include/hsr_losses.h: an out-of-range label matches no class and its pixel still counts.  Level widths 5 and 16 are held in registers
    (slots behind the level hold -inf: a label that picks one would make the loss +inf), 17 streams."""
    sizes, K, H, W = [5, 16, 17], 38, 19, 33
    g = np.random.default_rng(516)
    z = g.normal(0, 3, (K, H, W)).astype(np.float32)
    lab = np.stack([g.integers(0, n, (H, W)) for n in sizes]).astype(np.int64)
    lab[0, 0, :4] = -100
    for l, n in enumerate(sizes):
        planted = [v for v in (n, n + 3, 15, 16, 40, -1, -7) if not 0 <= v < n]
        for j, v in enumerate(planted):
            lab[l, 2 + l, 3 * j:3 * j + 2] = v                      # two pixels each, inside one wave
            lab[l, 12 + l, 30 - j] = v                              # and one in another block of 256
    _check_tree(z, lab, sizes, "out-of-range labels")


def test_out_of_range_labels_match_no_class_in_the_leaf_head():
    import loss_oracle as LO
    K, Cc, H, W, up = 7, 5, 23, 29, 1.75
    sem, w, b, lab = _leaf_data(K, Cc, H, W, 75)
    for j, v in enumerate((5, 15, 16, -1)):
        lab[3, 4 * j:4 * j + 3] = v
        lab[20, 28 - j] = v
    got = _leaf_fused(sem, w, b, lab, up)
    ref = LO.leaf_mlp_cross_entropy(sem, w, b, lab)
    e = _leaf_distances(got, ref, up)
    print("leaf, out-of-range labels: loss %.3e d_sem %.3e d_weight %.3e d_bias %.3e" % e)
    assert all(bool(torch.isfinite(x).all()) for x in got)
    assert e[0] < LEAF_LOSS_TOL * max(1.0, abs(ref[0])) and e[1] < LEAF_DSEM_TOL and e[2] < LEAF_DW_TOL and e[3] < LEAF_DW_TOL


# ---------------------------------------------------------------- large logits
def test_tree_ce_with_logits_of_plus_and_minus_80():
    """the max-subtraction of every path.  N(0, 3) logits; rows 0-5 carry one +80 per pixel and level (the other classes' softmax is ~e^-80),
    rows 6-11 one -80, rows 12-14 one whole level each at +80; rows 16 and 17 one +100 / -100 per pixel, where e^100 is past fp32's largest
    number: without the subtraction the sum is +inf"""
    sizes, K, H, W = [4, 16, 17], 37, 19, 33
    g = np.random.default_rng(80)
    z = g.normal(0, 3, (K, H, W)).astype(np.float32)
    lab = _tree_labels(g, sizes, H, W)
    b = 0
    for l, n in enumerate(sizes):
        for y in range(12):
            ch = g.integers(0, n, W)
            z[b + ch, y, np.arange(W)] = 80.0 if y < 6 else -80.0
        z[b:b + n, 12 + l] = 80.0
        for y, v in ((16, 100.0), (17, -100.0)):
            z[b + g.integers(0, n, W), y, np.arange(W)] = v
        b += n
    _check_tree(z, lab, sizes, "logits +-80")


# The leaf kernel evaluates exp2(z * log2(e) - lse2): one more rounding than exp(z - lse), on an argument 1.44 times as large, so its
# softmax error grows with |z|.  Bound: the larger of the bound at O(10) logits and FOUR times the distance of torch's fp32 chain on the
# device from the float64 oracle (measured in the test and printed by it).  The same chain in fp32 on the CPU (of the largest entry; no
# device figure has been taken yet, and none of the fused kernel: the test prints both):
#                                    d_sem      d_weight   d_bias
#   scaled, max |z| = 66.7   eager   1.2e-06    4.0e-07    2.2e-07
#   all logits < -89         eager   1.4e-06    2.3e-07    6.6e-07
@pytest.mark.parametrize("case", ["scaled", "all_below_minus_89"])
def test_leaf_head_with_large_logits(case):
    """scaled: K = 26, C = 102, weights x 4.5, logits to about +-60.  all_below_minus_89: K = 7, C = 5 with every bias at -100, so that
    2^(-lse2) of the 11 padding rows behind the last class is +inf in fp32: they must be masked, not multiplied by their zero weights."""
    import loss_oracle as LO
    H, W, up = 23, 29, 1.75
    if case == "scaled":
        K, Cc = 26, 102
        sem, w, b, lab = _leaf_data(K, Cc, H, W, 60, wscale=4.5)
    else:
        K, Cc = 7, 5
        sem, w, b, lab = _leaf_data(K, Cc, H, W, 89)
        b = (b - 100.0).astype(np.float32)
    z = w.astype(np.float64) @ sem.astype(np.float64).reshape(K, -1) + b.astype(np.float64)[:, None]
    if case == "scaled":
        assert 40.0 <= np.abs(z).max() <= 80.0, np.abs(z).max()
    else:
        assert z.max() < -89.0, z.max()             # 2^(89 log2 e) = e^89 > fp32's largest number
    got = _leaf_fused(sem, w, b, lab, up)
    ref = LO.leaf_mlp_cross_entropy(sem, w, b, lab)
    e = _leaf_distances(got, ref, up)
    q = _leaf_distances(_leaf_eager(sem, w, b, lab, up), ref, up)
    print("%s: z in [%.1f, %.1f], loss %.4f; fused: loss %.3e d_sem %.3e d_weight %.3e d_bias %.3e | eager: loss %.3e d_sem %.3e d_weight %.3e "
          "d_bias %.3e" % ((case, z.min(), z.max(), ref[0]) + e + q))
    assert all(bool(torch.isfinite(x).all()) for x in got)
    assert e[0] < LEAF_LOSS_TOL * max(1.0, abs(ref[0]))
    assert e[1] < max(LEAF_DSEM_TOL, 4 * q[1])
    assert e[2] < max(LEAF_DW_TOL, 4 * q[2]) and e[3] < max(LEAF_DW_TOL, 4 * q[3])


# ---------------------------------------------------------------- SSIM
@pytest.mark.parametrize("H,W", [(32, 32), (33, 33), (31, 65), (64, 32), (1, 1), (11, 11)])
def test_ssim_at_tile_edges(H, W):
    """the tile is 32 x 32: exactly one, one pixel into the next in both directions, one short / one past two, two stacked, one pixel, one
    window"""
    import loss_oracle as LO
    from hsr_utils import losses as L
    g = np.random.default_rng(H * W)
    x, y = g.random((1, H, W)).astype(np.float32), g.random((1, H, W)).astype(np.float32)
    tx = torch.tensor(x, device="cuda", requires_grad=True)
    s = L.calc_ssim(tx, torch.tensor(y, device="cuda"))
    s.backward()
    v, gr = LO.ssim(x, y)
    print("ssim %dx%d: value %.2e grad %.2e" % (H, W, abs(float(s) - v), _relmax(_np(tx.grad), gr)))
    assert abs(float(s) - v) < SSIM_VAL_TOL and _relmax(_np(tx.grad), gr) < SSIM_GRAD_TOL


def _ssim_fp32_formula_on_cpu(x, y):
    """the reference's formula in fp32 (torch conv2d on the CPU, as eager_ssim of test_losses_chained_behind_the_rasterizer): value, gradient"""
    import loss_oracle as LO
    import torch.nn.functional as F
    w = torch.tensor(LO.window_2d()).reshape(1, 1, 11, 11)
    a, b = torch.tensor(x).unsqueeze(0).requires_grad_(True), torch.tensor(y).unsqueeze(0)
    mu1, mu2 = F.conv2d(a, w, padding=5), F.conv2d(b, w, padding=5)
    s1 = F.conv2d(a * a, w, padding=5) - mu1 ** 2
    s2 = F.conv2d(b * b, w, padding=5) - mu2 ** 2
    s12 = F.conv2d(a * b, w, padding=5) - mu1 * mu2
    v = (((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 ** 2 + mu2 ** 2 + 1e-4) * (s1 + s2 + 9e-4))).mean()
    v.backward()
    return float(v.detach()), a.grad[0].numpy()


# img1 constant: sigma_1 = E[x^2] - mu^2 is all cancellation.  Bound on the gradient: the larger of SSIM_GRAD_TOL and twice the distance of
# the fp32 evaluation of the reference's formula (CPU) from the float64 oracle.  Measured at 33 x 65: the fp32 formula is 1.4e-06 of the
# largest entry away (value: 7.0e-07), so SSIM_GRAD_TOL is the bound that holds.
def test_ssim_of_a_zero_variance_image():
    import loss_oracle as LO
    from hsr_utils import losses as L
    H, W = 33, 65
    g = np.random.default_rng(5)
    x, y = np.full((1, H, W), 0.5, np.float32), g.random((1, H, W)).astype(np.float32)
    v, gr = LO.ssim(x, y)
    v32, g32 = _ssim_fp32_formula_on_cpu(x, y)
    d32 = _relmax(g32, gr)
    tx = torch.tensor(x, device="cuda", requires_grad=True)
    s = L.calc_ssim(tx, torch.tensor(y, device="cuda"))
    s.backward()
    print("zero-variance ssim: fp32 formula value %.2e grad %.2e; fused value %.2e grad %.2e" % (abs(v32 - v), d32, abs(float(s) - v),
                                                                                                 _relmax(_np(tx.grad), gr)))
    assert np.isfinite(_np(tx.grad)).all()
    assert abs(float(s) - v) < SSIM_VAL_TOL
    assert _relmax(_np(tx.grad), gr) < max(SSIM_GRAD_TOL, 2 * d32)
