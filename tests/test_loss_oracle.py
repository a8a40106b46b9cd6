"""CPU suite for the loss-head row: oracle/loss_oracle.py against the committed outputs of the
reference's own helpers (tests/golden/loss_ssim_l1.npz: calc_ssim and l1_loss_v1 imported from the reference, values and
autograd gradients) and of torch.nn.CrossEntropyLoss applied per tree level as the reference applies it."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import loss_oracle as LO  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SSIM_GRAD_TOL = 5e-4


@pytest.mark.parametrize("case", ["random_40x56", "smooth_68x120", "tiny_7x9"])
def test_ssim_and_l1_match_reference_outputs(case):
    d = np.load(os.path.join(GOLD, "loss_ssim_l1.npz"))
    x, y = d[case + "/img1"], d[case + "/img2"]
    v, g = LO.ssim(x, y)
    assert abs(v - float(d[case + "/ssim"])) < 2e-6
    ref_g = d[case + "/ssim_grad"]
    # the reference evaluates sigma = E[x^2] - mu^2 in fp32: on smooth images (sigma ~ 1e-3) that cancellation leaves its
    # own gradient ~2e-4 (relative to the largest entry) away from the float64 value; random images agree to 2e-6
    assert np.abs(g - ref_g).max() <= SSIM_GRAD_TOL * np.abs(ref_g).max()
    l, lg = LO.l1_mean(x, y)
    assert abs(l - float(d[case + "/l1"])) < 1e-6
    np.testing.assert_allclose(lg, d[case + "/l1_grad"], rtol=1e-6, atol=1e-12)


def test_window_is_the_reference_window():
    w = LO.window_2d()
    assert w.shape == (11, 11) and w.dtype == np.float32
    assert abs(float(w.sum()) - 1.0) < 1e-6 and np.array_equal(w, w.T) and np.array_equal(w, w[::-1, ::-1])


def test_tree_cross_entropy_matches_torch():
    d = np.load(os.path.join(GOLD, "loss_tree_ce.npz"))
    losses, grad = LO.tree_cross_entropy(d["logits"], d["labels"], list(d["level_sizes"]))
    np.testing.assert_allclose(losses, d["per_level"], rtol=2e-6)
    assert np.abs(grad - d["grad"]).max() <= 2e-6 * np.abs(d["grad"]).max()


@pytest.mark.parametrize("reduction", ["sum", "mean"])
def test_masked_l1_matches_torch_indexing(reduction):
    g = np.random.default_rng(3)
    pred, gt = g.random((3, 20, 30)).astype(np.float32), g.random((3, 20, 30)).astype(np.float32)
    mask = g.random((20, 30)) > 0.4
    tp = torch.tensor(pred, requires_grad=True)
    sel = torch.abs(torch.tensor(gt) - tp)[torch.tile(torch.tensor(mask), (3, 1, 1))]   # scripts/hierslam.py:933-935
    ref = sel.sum() if reduction == "sum" else sel.mean()
    ref.backward()
    loss, grad = LO.masked_l1(pred, gt, mask, reduction)
    assert abs(loss - float(ref)) <= 1e-5 * abs(float(ref))
    np.testing.assert_allclose(grad, tp.grad.numpy(), rtol=1e-6, atol=1e-12)


def test_leaf_mlp_head_matches_torch_fixture():
    d = np.load(os.path.join(GOLD, "loss_leaf_mlp.npz"))
    loss, ds, dw, db = LO.leaf_mlp_cross_entropy(d["sem"], d["weight"], d["bias"], d["labels"])
    assert abs(loss - float(d["loss"])) < 2e-6
    for got, key in ((ds, "d_sem"), (dw, "d_weight"), (db, "d_bias")):
        assert np.abs(got - d[key]).max() <= 3e-6 * np.abs(d[key]).max(), key


# ---------------------------------------------------------------- out-of-range labels and the edge layouts of tests/test_gpu_losses_edges.py
def _torch_tree_ce64(z, lab, sizes):
    """torch.nn.functional.cross_entropy per level in float64: (per-level losses, d sum / d logits)"""
    tz = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    K, H, W = z.shape
    losses, b = [], 0
    for l, n in enumerate(sizes):
        losses.append(torch.nn.functional.cross_entropy(tz[b:b + n].permute(1, 2, 0).reshape(-1, n), torch.tensor(lab[l]).reshape(-1)))
        b += n
    torch.stack(losses).sum().backward()
    return np.array([float(x) for x in losses]), tz.grad.numpy()


@pytest.mark.parametrize("sizes", [[1], [16], [17], list(range(1, 17))], ids=["one", "sixteen", "seventeen", "sixteen_levels"])
def test_tree_cross_entropy_matches_torch_float64_at_the_edge_layouts(sizes):
    g = np.random.default_rng(sum(sizes))
    K, H, W = sum(sizes), 7, 9
    z = g.normal(0, 3, (K, H, W))
    lab = np.stack([g.integers(0, n, (H, W)) for n in sizes]).astype(np.int64)
    lab[0, 0, :3] = -100
    want_l, want_g = _torch_tree_ce64(z, lab, sizes)
    got_l, got_g = LO.tree_cross_entropy(z, lab, sizes)
    np.testing.assert_allclose(got_l, want_l, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(got_g, want_g, rtol=1e-11, atol=1e-15)
    if sizes[0] == 1:
        assert got_l[0] == 0.0 and not got_g[0].any()           # a one-class level: loss 0 and gradient 0 exactly


def test_in_range_labels_are_untouched_by_the_out_of_range_rule():
    """the oracle as it stood before the rule (gather with the label, subtract the one-hot), restated, on in-range labels with
    ignored pixels: identical results, bit for bit; and the leaf head against torch float64."""
    g = np.random.default_rng(2)
    sizes, H, W = [3, 5], 6, 5
    z = g.normal(0, 2, (8, H, W))
    lab = np.stack([g.integers(0, n, (H, W)) for n in sizes]).astype(np.int64)
    lab[1, 2] = -100
    got_l, got_g = LO.tree_cross_entropy(z, lab, sizes)
    b = 0
    for l, n in enumerate(sizes):
        zl, la = z[b:b + n].reshape(n, -1), lab[l].reshape(-1)
        valid = la != -100
        m = zl.max(axis=0)
        e = np.exp(zl - m)
        lse = m + np.log(e.sum(axis=0))
        safe = np.where(valid, la, 0)
        assert got_l[l] == ((lse - zl[safe, np.arange(H * W)]) * valid).sum() / valid.sum()
        sm = e / e.sum(axis=0)
        sm[safe, np.arange(H * W)] -= 1.0
        assert np.array_equal(got_g[b:b + n], (sm * valid / valid.sum()).reshape(n, H, W))
        b += n
    K, C = 4, 6
    sem, w, bias = g.normal(0, 1, (K, H, W)), g.normal(0, 1, (C, K)), g.normal(0, 1, (C,))
    ll = g.integers(0, C, (H, W)).astype(np.int64)
    ll[0, :2] = -100
    ts, tw, tb = (torch.tensor(a, requires_grad=True) for a in (sem, w, bias))
    ref = torch.nn.functional.cross_entropy((tw @ ts.reshape(K, -1) + tb[:, None]).t(), torch.tensor(ll).reshape(-1))
    ref.backward()
    lo, ds, dw, db = LO.leaf_mlp_cross_entropy(sem, w, bias, ll)
    assert abs(lo - float(ref)) < 1e-13
    for got, want in ((ds, ts.grad), (dw, tw.grad), (db, tb.grad)):
        np.testing.assert_allclose(got, want.numpy(), rtol=1e-11, atol=1e-15)


def test_out_of_range_labels_follow_the_header_rule_on_a_3x4_map():
    """include/hsr_losses.h: an out-of-range label matches no class, and the pixel still counts toward the mean — written out by hand."""
    g = np.random.default_rng(4)
    n, H, W = 3, 3, 4
    z = g.normal(0, 2, (n, H, W))
    lab = g.integers(0, n, (H, W)).astype(np.int64)
    lab[0, 0], lab[0, 1], lab[1, 2], lab[2, 3], lab[2, 0] = 3, -1, 40, -7, -100     # four out of range, one ignored
    loss, grad, cnt = 0.0, np.zeros_like(z), 11
    for y in range(H):
        for x in range(W):
            if lab[y, x] == -100:
                continue
            p = np.exp(z[:, y, x]) / np.exp(z[:, y, x]).sum()
            lse = math.log(np.exp(z[:, y, x]).sum())
            if 0 <= lab[y, x] < n:
                loss += lse - z[lab[y, x], y, x]
                p[lab[y, x]] -= 1.0
            else:
                loss += lse
            grad[:, y, x] = p / cnt
    got_l, got_g = LO.tree_cross_entropy(z, lab[None], [n])
    assert abs(got_l[0] - loss / cnt) < 1e-14
    np.testing.assert_allclose(got_g, grad, rtol=1e-12, atol=1e-16)
    # the leaf head with identity weights and no bias is the same loss on the same logits
    lo, ds, dw, db = LO.leaf_mlp_cross_entropy(z, np.eye(n), np.zeros(n), lab)
    assert abs(lo - loss / cnt) < 1e-14
    np.testing.assert_allclose(ds, grad, rtol=1e-12, atol=1e-16)
    np.testing.assert_allclose(db, grad.reshape(n, -1).sum(axis=1), rtol=1e-12, atol=1e-16)
    np.testing.assert_allclose(dw, grad.reshape(n, -1) @ z.reshape(n, -1).T, rtol=1e-12, atol=1e-15)
