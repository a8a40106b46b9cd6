"""CPU suite for the map evaluation: the checker's boundary restatements agree with each other bit for bit, the host-only pieces of
hsr_utils/evaluate.py (trajectory ATE, tree lookup table) match the reference's semantics, and the host-only entry points of
include/hsr_eval.h answer and its prototypes are exported and bound with the right types (the one checker of tests/test_abi.py)."""
import numpy as np
import pytest
import torch

import eval_ref as R
from test_abi import check_header


def blob_labels(g, H, W, values, n_blobs=12):
    lab = np.full((H, W), values[0], np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    for _ in range(n_blobs):
        cy, cx = g.uniform(0, H), g.uniform(0, W)
        ry, rx = g.uniform(1, H / 2.5), g.uniform(1, W / 2.5)
        lab[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1] = g.choice(values)
    return lab


def label_maps():
    g = np.random.default_rng(3)
    for H, W in ((7, 9), (48, 64), (480, 640)):
        yield "random_%dx%d" % (H, W), g.integers(0, 4, (H, W))
        yield "blob_%dx%d" % (H, W), blob_labels(g, H, W, [0, 1, 2, 5, -1, 255])
    yield "single_48x64", np.full((48, 64), 3)
    yield "single_7x9", np.full((7, 9), 0)


def test_dilation_pixels():
    assert R.dilation_pixels(680, 1200) == 28 and R.dilation_pixels(480, 640) == 16 and R.dilation_pixels(7, 9) == 1
    from hsr_utils.evaluate import dilation_pixels
    for H, W in ((680, 1200), (480, 640), (7, 9), (25, 25), (1, 1), (3000, 4000)):
        assert dilation_pixels(H, W) == R.dilation_pixels(H, W)


@pytest.mark.parametrize("name,lab", list(label_maps()), ids=[n for n, _ in label_maps()])
def test_boundary_restatements_agree(name, lab):
    H, W = lab.shape
    d = R.dilation_pixels(H, W)
    flags = R.boundary_flags(lab, d)
    classes = np.unique(lab)
    # the literal cv2 recipe is slow at 480x640 (d = 16 iterations per class): every class there, but only through scipy for the rest
    literal = H * W <= 48 * 64 or name.startswith("blob")
    for c in classes:
        m = (lab == c).astype(np.uint8)
        win = (m.astype(bool) & flags).astype(np.uint8)
        sp = R.boundary_scipy(m, d)
        assert np.array_equal(sp, win), (name, c)
        if literal:
            assert np.array_equal(R.boundary_cv2(m, d), win), (name, c)


def test_counts_match_literal_loop():
    g = np.random.default_rng(5)
    for H, W in ((7, 9), (48, 64), (33, 70)):
        gt = blob_labels(g, H, W, [0, 1, 2, 3, 255])
        pred = np.where(g.random((H, W)) < 0.1, g.integers(0, 5, (H, W)), gt)
        classes = list(range(5))
        counts = R.iou_counts(pred, gt, classes)
        np.testing.assert_allclose(R.frame_miou(counts), R.frame_miou_literal(pred, gt, classes), rtol=0, atol=1e-12)


def test_frame_miou_no_class_is_nan():
    assert np.isnan(R.frame_miou(np.zeros((4, 6), np.int64))).all()


def _poses(g, n):
    out = []
    for _ in range(n):
        q = g.normal(size=4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                       [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                       [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = Rm, g.normal(size=3)
        out.append(T)
    return out


def test_trajectory_ate_rigid_copy_is_zero():
    from hsr_utils.evaluate import trajectory_ate
    g = np.random.default_rng(11)
    gt = _poses(g, 40)
    A = _poses(g, 1)[0]
    # the w2c [:3,3] columns moved by one rigid transform; frame 0's estimate is gt[0] by construction: keep it on the same map
    est = [A @ m for m in gt]
    gt_moved = [np.linalg.inv(A) @ m for m in est]
    assert trajectory_ate(gt_moved, est, first_frame_w2c=est[0]) < 1e-9


def test_trajectory_ate_matches_horn():
    from hsr_utils.evaluate import trajectory_ate
    g = np.random.default_rng(12)
    gt = _poses(g, 60)
    est = [m + np.pad(g.normal(0, 0.05, (3, 1)), ((0, 1), (3, 0))) for m in gt]
    gt[7] = np.full((4, 4), np.nan)
    gt[30][1, 2] = np.nan
    got = trajectory_ate([torch.tensor(m) for m in gt], est)
    assert abs(got - R.trajectory_ate(gt, est)) < 1e-12
    # a direct Horn solution (Umeyama without scale) over the frames kept
    keep = [0] + [i for i in range(1, 60) if not np.isnan(gt[i]).any()]
    P = np.stack([gt[i][:3, 3] for i in keep])
    Q = np.stack([gt[0][:3, 3]] + [est[i][:3, 3] for i in keep[1:]])
    mp, mq = P.mean(0), Q.mean(0)
    U, _s, Vt = np.linalg.svd((Q - mq).T @ (P - mp))
    D = np.diag([1, 1, np.sign(np.linalg.det(U @ Vt))])
    Rm = U @ D @ Vt
    err = np.linalg.norm((P - mp) @ Rm.T + mq - Q, axis=1).mean()
    assert abs(got - err) < 1e-10


def test_tree_lookup_table_missing_and_duplicate():
    from hsr_utils.evaluate import tree_lookup_table
    sizes = [2, 3, 4, 99]                       # three levels + the leaf count
    mapping = {"5": (0, 1, 2), "7": (1, 2, 3), "9": (0, 1, 2), 11: (1, 0, 0), "13": (1, 5, 0)}   # "9" repeats "5"'s tuple; "13" out of range
    t = tree_lookup_table(mapping, sizes, device="cpu").numpy()
    assert t.dtype == np.int32 and t.shape == (24,)
    levels = np.array(np.meshgrid(np.arange(2), np.arange(3), np.arange(4), indexing="ij")).reshape(3, -1)
    expect = R.tree_to_leaf(levels.reshape(3, 1, 24), mapping).reshape(-1)
    idx = (levels[0] * 3 + levels[1]) * 4 + levels[2]
    assert np.array_equal(t[idx], expect)
    assert t[(0 * 3 + 1) * 4 + 2] == 9 and t[(1 * 3 + 0) * 4 + 0] == 11 and (t == -1).sum() == 21


def test_eval_abi_exported_and_bound():
    assert {"hsr_eval_frame_metrics", "hsr_eval_labels_flat", "hsr_eval_labels_tree", "hsr_eval_labels_leaf", "hsr_eval_iou_counts",
            "hsr_eval_frame_miou", "hsr_eval_metrics_scratch_bytes", "hsr_eval_leaf_scratch_bytes",
            "hsr_eval_iou_scratch_bytes"} <= set(check_header("hsr_eval.h"))


def test_scratch_sizes_host_only():
    from hsr_utils import evaluate as E
    assert E._lib.hsr_eval_iou_scratch_bytes(680, 1200) >= 2 * 4 * 680 * 1200
    assert E._lib.hsr_eval_leaf_scratch_bytes(102) >= 102 * 33 * 4
    assert E._lib.hsr_eval_metrics_scratch_bytes(680, 1200) > 0


def test_cpu_tensors_are_refused():
    from hsr_utils import evaluate as E
    x = torch.zeros(3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.frame_metrics(x, x, x[0], x[0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.iou_counts(torch.zeros(8, 8, dtype=torch.int32), torch.zeros(8, 8, dtype=torch.int32), num_classes=3)
