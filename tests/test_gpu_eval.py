"""GPU parity for the map evaluation (include/hsr_eval.h, hsr_utils/evaluate.py): frame metrics against the committed outputs of the
reference's own calc_psnr and depth lines (tests/golden/eval/psnr_depth.npz; a directory of its own, out of the
rasterizer fixtures that tests/test_oracle.py collects from tests/golden/*.npz) and float64 numpy, labels against torch's
argmax(softmax) on the same device, per-class counts bit-exact against tests/eval_ref.py, and one rendered frame end to end."""
import os

import numpy as np
import pytest
import torch

import eval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.gpu

PSNR_TOL = 1e-4       # dB
DEPTH_TOL = 2e-6      # relative: fp32 per thread over 4 pixels, double from there on
TREE_SIZES = [2, 4, 6, 6, 8, 102]   # the suite's K = 26 five-level split + the leaf count (the dataset's num_semantic)


def _ev():
    from hsr_utils import evaluate as E
    return E


def _check_metrics(got, exp):
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    if np.isinf(exp[0]):
        assert np.isinf(got[0]) and got[0] > 0
    else:
        assert abs(got[0] - exp[0]) < PSNR_TOL, (got, exp)
    for k in (1, 2):
        if np.isnan(exp[k]):
            assert np.isnan(got[k])
        else:
            assert abs(got[k] - exp[k]) <= DEPTH_TOL * abs(exp[k]), (k, got, exp)


@pytest.mark.parametrize("case", ["sil_64x80", "nosil_37x53", "exact_g_48x64"])
def test_frame_metrics_match_reference_outputs(case):
    E = _ev()
    d = np.load(os.path.join(GOLD, "eval", "psnr_depth.npz"))
    g = lambda k: torch.tensor(d[case + "/" + k]).cuda()
    use_sil = bool(d[case + "/use_sil"])
    got = E.frame_metrics(g("im"), g("gt_im"), g("depth"), g("gt_depth"), g("final_opacity") if use_sil else None,
                          float(d[case + "/sil_thres"]) if use_sil else None).cpu().numpy()
    exp = d[case + "/expect"]                   # the reference's fp32 values
    assert (np.isinf(got[0]) and np.isinf(exp[0])) or abs(got[0] - exp[0]) < PSNR_TOL, (got, exp)
    np.testing.assert_allclose(got[1:], exp[1:], rtol=1e-5)
    f64 = R.frame_metrics(*(d[case + "/" + k] for k in ("im", "gt_im", "depth", "gt_depth")),
                          d[case + "/final_opacity"] if use_sil else None, float(d[case + "/sil_thres"]) if use_sil else None)
    _check_metrics(got, f64)


@pytest.mark.parametrize("H,W", [(1, 1), (7, 9), (33, 47), (257, 129), (680, 1200)])
@pytest.mark.parametrize("use_sil", [False, True])
def test_frame_metrics_float64_and_repeatable(H, W, use_sil):
    E = _ev()
    g = torch.Generator().manual_seed(H * 1000 + W + use_sil)
    gt_im = torch.rand(3, H, W, generator=g)
    im = (gt_im + 0.05 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    gt_d = torch.rand(1, H, W, generator=g) * 5 + 0.5
    gt_d[torch.rand(1, H, W, generator=g) < 0.2] = 0
    if H * W == 1:
        gt_d[:] = 1.0
    d = gt_d + 0.1 * torch.randn(1, H, W, generator=g)
    op = torch.rand(1, H, W, generator=g)
    args = [t.cuda() for t in (im, gt_im, d, gt_d)] + ([op.cuda(), 0.4] if use_sil else [None, None])
    a, b = E.frame_metrics(*args), E.frame_metrics(*args)
    assert torch.equal(a, b)
    exp = R.frame_metrics(im.numpy(), gt_im.numpy(), d.numpy(), gt_d.numpy(), op.numpy() if use_sil else None, 0.4 if use_sil else None)
    _check_metrics(a.cpu().numpy(), exp)


def test_frame_metrics_inf_and_nan():
    E = _ev()
    H, W = 40, 70
    im = torch.rand(3, H, W, device="cuda")
    d = torch.rand(1, H, W, device="cuda") + 1
    r = E.frame_metrics(im, im.clone(), d, d.clone()).cpu().numpy()
    assert np.isinf(r[0]) and r[0] > 0 and r[1] == 0 and r[2] == 0
    r = E.frame_metrics(im, torch.rand(3, H, W, device="cuda"), d, torch.zeros(1, H, W, device="cuda")).cpu().numpy()
    # no valid depth: every image term is masked to 0 -> mse 0 -> +inf; depth 0/0 -> NaN
    assert np.isinf(r[0]) and np.isnan(r[1]) and np.isnan(r[2])


def _near_tie_ok(z, got, axis_logits):
    """pixels where `got` differs from torch.argmax(torch.softmax(z)): allowed only where torch's top two probabilities are equal or
    adjacent floats (`axis_logits`: the class axis of z).  Returns (mismatches, unexplained)."""
    p = torch.softmax(z, dim=axis_logits)
    ref = torch.argmax(p, dim=axis_logits).to(torch.int32)
    bad = ref != got
    n = int(bad.sum())
    if n == 0:
        return 0, 0
    top2 = torch.topk(p, 2, dim=axis_logits).values
    p1, p2 = top2.select(axis_logits, 0), top2.select(axis_logits, 1)
    adjacent = torch.nextafter(p2, torch.full_like(p2, float("inf"))) >= p1
    return n, int((bad & ~adjacent).sum())


@pytest.mark.parametrize("H,W", [(7, 9), (680, 1200)])
def test_labels_flat(H, W):
    E = _ev()
    g = torch.Generator().manual_seed(3)
    z = (torch.randn(26, H, W, generator=g) * 3).cuda()
    z[:, 0, :] = 0.0                                  # exact ties across all 26 classes: index 0
    z[:, -1, :] = -5.0
    z[4, -1, :], z[9, -1, :] = 2.0, 2.0               # exact tie of two: index 4
    lab = E.semantic_labels(z, "flat")
    assert lab.dtype == torch.int32 and lab.shape == (H, W)
    assert (lab[0] == 0).all() and (lab[-1] == 4).all()
    n, unexplained = _near_tie_ok(z, lab, 0)
    print("flat %dx%d: %d pixels differ from torch, all at equal / adjacent top probabilities" % (H, W, n))
    assert unexplained == 0


def _tree_mapping(g):
    sizes = TREE_SIZES[:-1]
    mapping = {}
    for leaf in range(TREE_SIZES[-1]):
        mapping[str(leaf)] = tuple(int(g.integers(0, s)) for s in sizes)
    mapping["40"] = mapping["3"]                      # a duplicate tuple: the later key wins
    return mapping


def test_labels_tree():
    E = _ev()
    H, W = 680, 1200
    g = np.random.default_rng(9)
    mapping = _tree_mapping(g)
    table = E.tree_lookup_table(mapping, TREE_SIZES)
    z = torch.tensor((g.normal(0, 2.0, (26, H, W))).astype(np.float32)).cuda()
    leaf, levels = E.semantic_labels(z, "tree", level_sizes=TREE_SIZES, tree_table=table)
    assert leaf.shape == (H, W) and levels.shape == (5, H, W)
    b, total = 0, 0
    for l, n in enumerate(TREE_SIZES[:-1]):
        m, unexplained = _near_tie_ok(z[b:b + n], levels[l], 0)
        assert unexplained == 0, l
        total += m
        b += n
    print("tree: %d level labels differ from torch, all at equal / adjacent top probabilities" % total)
    # the leaf id is the Python dict restatement of transfer_tree_2_label applied to these level labels, exactly
    exp = R.tree_to_leaf(levels.cpu().numpy(), mapping)
    assert np.array_equal(leaf.cpu().numpy(), exp)
    assert (exp == -1).any() and (exp == 40).any() and not (exp == 3).any()


def test_labels_leaf():
    E = _ev()
    H, W, K, Cc = 680, 1200, 26, 102
    torch.manual_seed(4)
    mlp = torch.nn.Conv2d(K, Cc, kernel_size=1).cuda()
    sem = torch.rand(K, H, W, device="cuda")
    lab = E.semantic_labels(sem, "leaf", mlp=mlp)
    with torch.no_grad():
        logits = mlp(sem.unsqueeze(0)).squeeze(0)
    p = torch.softmax(logits, 0)
    ref = torch.argmax(p, 0).to(torch.int32)
    bad = ref != lab
    top2 = torch.topk(p, 2, dim=0).values
    # our logits are a 32-term fp32 FMA chain, torch's a convolution: a differing pixel must be a near tie of torch's probabilities
    near = (top2[0] - top2[1]) <= 1e-5 * top2[0]
    print("leaf K=26 C=102: %d of %d pixels differ from torch, all near ties" % (int(bad.sum()), H * W))
    assert int((bad & ~near).sum()) == 0
    assert int(bad.sum()) <= 20
    # a (weight, bias) pair works as the module does
    assert torch.equal(E.semantic_labels(sem, "leaf", mlp=(mlp.weight, mlp.bias)), lab)


def _maps(kind, H, W, values, seed):
    g = np.random.default_rng(seed)
    if kind == "random":
        gt = g.choice(values, (H, W))
        pred = g.choice(values, (H, W))
    else:
        gt = np.full((H, W), values[0], np.int64)
        yy, xx = np.mgrid[0:H, 0:W]
        for _ in range(40):
            cy, cx, ry, rx = g.uniform(0, H), g.uniform(0, W), g.uniform(1, H / 3), g.uniform(1, W / 3)
            gt[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1] = g.choice(values)
        pred = gt.copy()
        for _ in range(15):
            cy, cx, ry, rx = g.uniform(0, H), g.uniform(0, W), g.uniform(1, H / 5), g.uniform(1, W / 5)
            pred[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1] = g.choice(values)
    return pred.astype(np.int32), gt.astype(np.int32)


CASES = [("random", 7, 9, 1), ("blob", 7, 9, 41), ("random", 480, 640, 41), ("blob", 480, 640, 102), ("blob", 680, 1200, 102),
         ("random", 680, 1200, 4096), ("blob", 680, 1200, 1), ("blob", 480, 640, 4096)]


@pytest.mark.parametrize("kind,H,W,C", CASES)
def test_iou_counts_bit_exact(kind, H, W, C):
    E = _ev()
    # labels include values outside the class set (-1, 255 when C < 255, C itself)
    values = list(range(min(C, 60))) + [-1, 255, C] + ([C - 1] if C > 60 else [])
    pred, gt = _maps(kind, H, W, values, seed=H + C)
    counts = E.iou_counts(torch.tensor(pred).cuda(), torch.tensor(gt).cuda(), num_classes=C)
    assert counts.dtype == torch.int64 and counts.shape == (C, 6)
    exp = R.iou_counts(pred, gt, list(range(C)))
    assert np.array_equal(counts.cpu().numpy(), exp)
    again = E.iou_counts(torch.tensor(pred).cuda(), torch.tensor(gt).cuda(), num_classes=C)
    assert torch.equal(again, counts)
    np.testing.assert_allclose(E.frame_miou(counts).cpu().numpy(), R.frame_miou(exp), rtol=0, atol=1e-12)


def test_iou_counts_sparse_class_ids():
    E = _ev()
    H, W = 480, 640
    ids = [1, 3, 7, 40, 1000, 5, 2 ** 20, -7, 255, 100000]       # arbitrary order, negative and large ids
    pred, gt = _maps("blob", H, W, ids + [0, 2, 999], seed=77)     # 0, 2, 999: in no class
    counts = E.iou_counts(torch.tensor(pred).cuda(), torch.tensor(gt).cuda(), class_ids=ids)
    exp = R.iou_counts(pred, gt, ids)
    assert np.array_equal(counts.cpu().numpy(), exp)
    np.testing.assert_allclose(E.frame_miou(counts).cpu().numpy(), R.frame_miou(exp), rtol=0, atol=1e-12)


def test_frame_miou_without_classes_is_nan():
    E = _ev()
    lab = torch.full((30, 40), 9, dtype=torch.int32, device="cuda")
    r = E.frame_miou(E.iou_counts(lab, lab, num_classes=5)).cpu().numpy()
    assert np.isnan(r).all()


def test_evaluate_frame_end_to_end():
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer_semantic
    from hsr_utils.camera import replica_intrinsics, setup_camera_tensors
    from hsr_utils.synthetic import make_scene
    E = _ev()
    W, H, K, P = 1200, 680, 26, 60000
    k = replica_intrinsics(W, H)
    cam = setup_camera_tensors(W, H, k, np.eye(4))
    sc = make_scene(P, W, H, K, k, seed=5, kind="slam", scale_mult=3.0)
    dev = torch.device("cuda:0")
    cam = GaussianRasterizationSettings(**{kk: (v.to(dev) if isinstance(v, torch.Tensor) else v) for kk, v in cam.items()})
    with torch.no_grad():
        im, _radii, sem, depth, _median, opac = GaussianRasterizer_semantic(cam)(
            means3D=sc["means3D"].to(dev), means2D=torch.zeros(P, 3, device=dev), opacities=sc["opacities"].to(dev),
            colors_precomp=sc["colors_precomp"].to(dev), scales=sc["scales"].to(dev), rotations=sc["rotations"].to(dev),
            semantics_precomp=(sc["semantics_precomp"] * 6).to(dev))
    g = torch.Generator().manual_seed(6)
    gt_im = (im.cpu() + 0.03 * torch.randn(3, H, W, generator=g)).clamp(0, 1).to(dev)
    gt_d = (depth.cpu() * (1 + 0.02 * torch.randn(1, H, W, generator=g))).to(dev)
    gt_d[:, :30] = 0
    rng = np.random.default_rng(8)
    mapping = _tree_mapping(rng)
    table = E.tree_lookup_table(mapping, TREE_SIZES)
    mlp = torch.nn.Conv2d(K, TREE_SIZES[-1], kernel_size=1).to(dev)
    host = {n: t.detach().cpu().numpy() for n, t in (("im", im), ("gt_im", gt_im), ("depth", depth), ("gt_depth", gt_d), ("opac", opac),
                                                     ("sem", sem))}
    for mode in ("tree", "leaf"):
        lab = E.semantic_labels(sem, mode, level_sizes=TREE_SIZES, tree_table=table, mlp=mlp)
        lab = lab[0] if mode == "tree" else lab
        gt_lab = lab.cpu().numpy().copy()
        gt_lab[rng.random((H, W)) < 0.05] = rng.integers(0, TREE_SIZES[-1])
        gt_lab[200:300, 400:700] = 17
        gt_t = torch.tensor(gt_lab, dtype=torch.int64, device=dev)       # the dataset's label maps are int64
        for sil in (False, True):
            kw = dict(final_opacity=opac, sil_thres=0.5) if sil else {}
            out = E.evaluate_frame(im, gt_im, depth, gt_d, sem, gt_t, mode, level_sizes=TREE_SIZES, tree_table=table, mlp=mlp,
                                   num_classes=TREE_SIZES[-1], **kw)
            assert all(v.is_cuda and v.dim() == 0 for v in out.values())
            m = R.frame_metrics(host["im"], host["gt_im"], host["depth"], host["gt_depth"], host["opac"] if sil else None, 0.5 if sil else None)
            _check_metrics([out["psnr"].item(), out["depth_l1"].item(), out["depth_rmse"].item()], m)
            # labels: the host restatement of the same rendered map; counts and scores from the labels the frame was scored with
            if mode == "tree":
                ref_lab = R.tree_to_leaf(R.tree_level_labels(host["sem"], TREE_SIZES), mapping)
            else:
                wt = mlp.weight.detach().cpu().numpy().reshape(TREE_SIZES[-1], K)
                z = np.einsum("ck,khw->chw", wt.astype(np.float64), host["sem"].astype(np.float64)) + mlp.bias.detach().cpu().numpy()[:, None, None]
                ref_lab = R.softmax_argmax(z.astype(np.float32))
            differ = int((ref_lab != lab.cpu().numpy()).sum())
            print("%s: %d of %d labels differ from the host restatement" % (mode, differ, H * W))
            assert differ <= 50
            counts = R.iou_counts(lab.cpu().numpy(), gt_lab, list(range(TREE_SIZES[-1])))
            s = R.frame_miou(counts)
            assert abs(out["miou"].item() - s[0]) < 1e-12 and abs(out["mbiou"].item() - s[1]) < 1e-12
            s_host = R.frame_miou(R.iou_counts(ref_lab, gt_lab, list(range(TREE_SIZES[-1]))))
            assert abs(out["miou"].item() - s_host[0]) < 1e-3 and abs(out["mbiou"].item() - s_host[1]) < 1e-3


def test_argument_checks():
    E = _ev()
    x = torch.rand(3, 8, 8, device="cuda")
    d = torch.rand(1, 8, 8, device="cuda")
    lab = torch.zeros(8, 8, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.frame_metrics(x.cpu(), x, d, d)
    with pytest.raises(RuntimeError, match="float32"):
        E.frame_metrics(x.double(), x, d, d)
    with pytest.raises(RuntimeError):
        E.frame_metrics(x[:2], x[:2], d, d)
    with pytest.raises(RuntimeError):
        E.frame_metrics(x, x, torch.rand(1, 8, 9, device="cuda"), d)
    with pytest.raises(RuntimeError):
        E.frame_metrics(x, x, d, d, final_opacity=d)
    with pytest.raises(RuntimeError, match="int32"):
        E.iou_counts(lab.long(), lab, num_classes=3)
    with pytest.raises(RuntimeError, match="4096"):
        E.iou_counts(lab, lab, num_classes=4097)
    with pytest.raises(RuntimeError):
        E.iou_counts(lab, lab, class_ids=[1, 2, 2])
    with pytest.raises(RuntimeError):
        E.iou_counts(lab, lab[:4], num_classes=3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.semantic_labels(torch.rand(5, 8, 8), "flat")
    with pytest.raises(RuntimeError):
        E.semantic_labels(torch.rand(5, 8, 8, device="cuda"), "nope")
    with pytest.raises(RuntimeError):
        E.semantic_labels(torch.rand(5, 8, 8, device="cuda"), "tree", level_sizes=[2, 4, 9], tree_table=torch.zeros(8, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="K <= 32"):
        E.semantic_labels(torch.rand(40, 8, 8, device="cuda"), "leaf", mlp=torch.nn.Conv2d(40, 5, 1).cuda())
    with pytest.raises(RuntimeError):
        E.frame_miou(torch.zeros(3, 5, dtype=torch.int64, device="cuda"))
