"""GPU suite for the scoring of a run's mesh (include/eval/hsr_mesh_eval.h, hsr_utils.mesh_eval): every kernel against the numpy
restatement of tests/mesh_eval_ref.py, bit for bit unless said otherwise, at the smallest sizes at which it can go wrong; the metrics
against the restatement's from the same squared distances; and the whole evaluation on the six-frame sequence of
tests/test_gpu_slam_session.py, the run that tests/test_gpu_mesh_run.py meshes, built afresh here."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_eval_ref as R
import test_gpu_slam_session as TS
from test_gpu_slam_session import sequence  # noqa: F401  (the fixture: six rendered frames of a hidden map)

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN, INF = float("nan"), float("inf")


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV) if dtype is None else torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(dtype)


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- areas and sampler --------------------------------------------------------------------------------------------------------------------
def device_sample(vertices, faces, S, seed, labels=None):
    """(area, cum, points, face, label | None) as numpy arrays: hsr_mesh_areas, torch.cumsum and hsr_mesh_sample called one by one"""
    from diff_gaussian_rasterization import _abi
    from hsr_utils import mesh_eval
    v, f = dev(vertices, torch.float32), dev(faces, torch.int32)
    lab = None if labels is None else dev(labels, torch.int32)
    area = mesh_eval.face_areas(v, f)
    cum = torch.cumsum(area.double(), 0)
    points = torch.full((S, 3), -7.0, device=DEV)
    face = torch.full((S,), -7, dtype=torch.int32, device=DEV)
    out_label = None if lab is None else torch.full((S,), -7, dtype=torch.int32, device=DEV)
    _abi.call(_abi.lib.hsr_mesh_sample, "hsr_mesh_sample", v.device, len(vertices), len(faces), S, seed, v.data_ptr(), f.data_ptr(), cum.data_ptr(),
              None if lab is None else lab.data_ptr(), points.data_ptr(), face.data_ptr(), None if lab is None else out_label.data_ptr())
    return (area.cpu().numpy(), cum.cpu().numpy(), points.cpu().numpy(), face.cpu().numpy(), None if lab is None else out_label.cpu().numpy())


def check_sample(vertices, faces, S, seed, labels=None):
    area, cum, points, face, label = device_sample(vertices, faces, S, seed, labels)
    want_area = R.areas(vertices, faces)
    assert np.array_equal(bits(area), bits(want_area))
    # the one float tolerance: the device's running sum and numpy's add in different orders (float64, fewer than 10^4 terms)
    assert np.allclose(cum, np.cumsum(want_area.astype(np.float64)), rtol=1e-12, atol=0)
    want = R.sample(vertices, faces, cum, S, seed, labels)      # fed the device's own cum
    assert np.array_equal(bits(points), bits(want[0])) and np.array_equal(face, want[1])
    assert (label is None and want[2] is None) or np.array_equal(label, want[2])
    assert (area[face] > 0).all()      # a face without area is never chosen
    return area, points, face, label


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_three_face_mesh_areas_and_samples(seed):
    area, points, face, label = check_sample(R.TRI_VERTICES, R.TRI_FACES, 4096, seed, R.TRI_LABELS)
    assert area.tolist() == [1.0, 0.0, 3.0]
    assert not (face == 1).any()
    n0 = int((face == 0).sum())
    print("seed %d: face 0 chosen %d times of 4096" % (seed, n0))
    assert 1024 - 111 <= n0 <= 1024 + 111      # 4 binomial standard deviations of 27.7
    assert n0 == [1013, 1066, 1040, 1014][seed]


def test_sampler_edges():
    g = np.random.default_rng(3)
    check_sample(R.TRI_VERTICES, R.TRI_FACES, 1, 5, R.TRI_LABELS)                      # S = 1
    check_sample(R.TRI_VERTICES, R.TRI_FACES[:1], 333, 6)                               # one face, no labels
    check_sample(R.TRI_VERTICES, R.TRI_FACES[2:], 65, 2 ** 64 - 1, R.TRI_LABELS)        # the largest seed: the counter wraps
    vertices = g.standard_normal((170, 3)).astype(np.float32)
    faces = g.integers(0, 170, (301, 3)).astype(np.int32)                               # F = 301, S = 1000: no multiple of 64 or 256
    faces[7], faces[300], faces[120] = (0, 1, 170), (-1, 2, 3), (5, 5, 9)               # out of range twice, and a degenerate face
    area, _points, face, _label = check_sample(vertices, faces, 1000, 11, g.integers(-1, 9, 170).astype(np.int32))
    assert area[[7, 300, 120]].tolist() == [0, 0, 0] and not np.isin(face, [7, 300, 120]).any() and len(np.unique(face)) > 200
    huge = np.array([[0, 0, 0], [3e38, 0, 0], [0, 3e38, 0], [1, 0, 0], [0, 1, 0]], np.float32)      # an area that is not finite counts as 0
    area, _points, face, _label = check_sample(huge, np.array([[0, 1, 2], [0, 3, 4]], np.int32), 70, 1)
    assert area.tolist() == [0.0, 0.5] and (face == 1).all()


def test_sample_mesh_is_the_same_chain_and_refuses_a_mesh_without_area():
    from hsr_utils import mesh_eval
    v, f, lab = dev(R.TRI_VERTICES), dev(R.TRI_FACES), dev(R.TRI_LABELS)
    points, face, labels = mesh_eval.sample_mesh(v, f, 500, seed=9, labels=lab)
    _area, _cum, want_points, want_face, want_label = device_sample(R.TRI_VERTICES, R.TRI_FACES, 500, 9, R.TRI_LABELS)
    assert np.array_equal(bits(points), bits(want_points)) and np.array_equal(face.cpu().numpy(), want_face)
    assert np.array_equal(labels.cpu().numpy(), want_label) and mesh_eval.sample_mesh(v, f, 500, seed=9)[2] is None
    with pytest.raises(ValueError, match="total area of 0"):
        mesh_eval.sample_mesh(v, f[1:2], 10)
    with pytest.raises(ValueError, match="no faces"):
        mesh_eval.sample_mesh(v, f[:0], 10)


# ---- nearest neighbour --------------------------------------------------------------------------------------------------------------------
FIXTURES = R.nn_fixtures()
_BRUTE = {}


def brute(name):
    """computed once per fixture and shared"""
    if name not in _BRUTE:
        queries, targets, _cell = FIXTURES[name]
        _BRUTE[name] = R.brute_nn(queries, targets)
    return _BRUTE[name]


@pytest.mark.parametrize("name", list(FIXTURES))
def test_nearest_neighbour_equals_brute_force(name):
    from hsr_utils import mesh_eval
    queries, targets, cell = FIXTURES[name]
    grid = mesh_eval.NearestGrid(dev(targets), cell)
    origin, c, dims = R.grid_of(targets, cell)
    assert (grid.origin, grid.cell, grid.dims) == (origin, c, dims)
    cells = grid._cells(dev(targets)).cpu().numpy()
    assert np.array_equal(cells, R.cells(targets, origin, c, dims))
    start = grid.cell_start.cpu().numpy()
    assert start[0] == 0 and start[-1] == len(targets) and (np.diff(start) == np.bincount(cells, minlength=int(np.prod(dims)))).all()
    order = np.argsort(cells, kind="stable")
    packed = grid.packed.cpu().numpy()
    assert np.array_equal(packed[:, :3].view(np.uint32), targets[order].view(np.uint32)) and np.array_equal(packed[:, 3].view(np.int32), order)
    d2, index = grid.query(dev(queries))
    want_d2, want_index = brute(name)
    assert d2.dtype == torch.float32 and index.dtype == torch.int32
    assert np.array_equal(bits(d2), bits(want_d2)) and np.array_equal(index.cpu().numpy(), want_index)
    if name == "hand_first_hit":
        assert index.tolist() == [1]      # the neighbour across the face, not the one in the query's own cell


def test_grid_grows_its_cell_to_the_limits():
    """a cell far too small for the box is grown in 2 % steps until the sides and the product fit; the answers stay brute force's"""
    from hsr_utils import mesh_eval
    queries, targets, _cell = FIXTURES["uniform_c0.1"]
    grid = mesh_eval.NearestGrid(dev(targets), 1e-4)
    assert (grid.origin, grid.cell, grid.dims) == R.grid_of(targets, 1e-4)
    assert max(grid.dims) <= 1024 and 2 ** 24 / 1.1 < int(np.prod(grid.dims)) <= 2 ** 24 and grid.cell > 1e-4      # one 2 % step is 6 % of cells
    d2, index = grid.query(dev(queries[:200]))
    want_d2, want_index = brute("uniform_c0.1")
    assert np.array_equal(bits(d2), bits(want_d2[:200])) and np.array_equal(index.cpu().numpy(), want_index[:200])
    assert grid.query(torch.zeros((0, 3), device=DEV))[0].shape == (0,)


# ---- seen ---------------------------------------------------------------------------------------------------------------------------------
K = np.array([[8.0, 0, 3.5], [0, 8.0, 2.5], [0, 0, 1]])
SH, SW = 6, 8


def device_seen(points, w2cs, depths=None, eps=0.0):
    from hsr_utils import mesh_eval
    got = mesh_eval.seen_vertices(dev(points, torch.float32), np.asarray(w2cs, np.float32), K, SH, SW, None if depths is None else [dev(d) for d in depths], eps)
    assert got.dtype == torch.bool
    return got.cpu().numpy().astype(np.uint8)


def test_seen_borders_and_behind_the_camera():
    pts = np.array([[0, 0, 1], [0, 0, -1], [0, 0, 0], [-0.5, 0, 1], [-0.5001, 0, 1], [0.4999, 0, 1], [0.5, 0, 1], [0, -0.375, 1], [0, -0.3751, 1],
                    [0, 0.3749, 1], [0, 0.375, 1], [NAN, 0, 1], [1e30, 0, 1], [0, 0, INF]], np.float32)
    want = R.seen(pts, np.eye(4), K, SH, SW)
    assert want.tolist() == [1, 0, 0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0]
    assert np.array_equal(device_seen(pts, [np.eye(4)]), want)      # depth = None
    assert device_seen(pts[:1], [np.eye(4)]).tolist() == [1] and device_seen(pts[1:2], [np.eye(4)]).tolist() == [0]      # V = 1


def test_seen_against_a_depth_image():
    depth = np.full((SH, SW), 0.9, np.float32)
    depth[3, 0], depth[3, 1], depth[3, 2] = 0.0, NAN, INF
    edge = np.float32(0.9) + np.float32(0.05)      # d + eps as the kernel adds it
    cols = lambda u, z: (u - 3.5) / 8.0 * z      # the x that lands in column u at depth z
    pts = np.array([[0, 0, 0.5], [0, 0, edge], [0, 0, np.nextafter(edge, np.float32(2))], [0, 0, edge - np.float32(0.05)], [0, 0, 2.0],
                    [cols(0, 0.5), 0, 0.5], [cols(1, 0.5), 0, 0.5], [cols(2, 0.5), 0, 0.5], [cols(3, 0.5), 0, 0.5]], np.float32)
    want = R.seen(pts, np.eye(4), K, SH, SW, depth, 0.05)
    assert want.tolist() == [1, 1, 0, 1, 0, 0, 0, 0, 1]      # in front, exactly d + eps, just behind it, eps in front of it, far behind; depth 0, NaN, +inf
    assert np.array_equal(device_seen(pts, [np.eye(4)], [depth], 0.05), want)
    assert device_seen(pts, [np.eye(4)], [depth[None]], 0.0).tolist() == R.seen(pts, np.eye(4), K, SH, SW, depth, 0.0).tolist()


def test_seen_accumulates_over_views_and_clears_nothing():
    import scenes
    g = np.random.default_rng(5)
    pts = (g.standard_normal((300, 3)) * [0.6, 0.5, 1.5] + [0, 0, 1.0]).astype(np.float32)      # V = 300: no multiple of 256
    tilted = scenes.tilted_w2c().astype(np.float32)
    depths = [g.uniform(0.5, 2.5, (SH, SW)).astype(np.float32) for _ in range(2)]
    first = R.seen(pts, np.eye(4), K, SH, SW, depths[0], 0.02)
    both = R.seen(pts, tilted, K, SH, SW, depths[1], 0.02, out=first)
    assert 0 < first.sum() < both.sum() < 300 and (both >= first).all()
    assert np.array_equal(device_seen(pts, [np.eye(4)], depths[:1], 0.02), first)
    assert np.array_equal(device_seen(pts, [np.eye(4), tilted], depths, 0.02), both)
    assert np.array_equal(device_seen(pts, [np.eye(4), tilted]), R.seen(pts, tilted, K, SH, SW, out=R.seen(pts, np.eye(4), K, SH, SW)))
    # general cameras as further views (scenes.CAMERAS: every entry of the rotation that hsr_camera_point reads is live), each with a depth
    # image of its own, on top of the two above
    cams = [m.astype(np.float32) for m in scenes.CAMERAS.values()]
    more = [g.uniform(0.5, 2.5, (SH, SW)).astype(np.float32) for _ in cams]
    want, plain, grew = both.copy(), R.seen(pts, tilted, K, SH, SW, out=R.seen(pts, np.eye(4), K, SH, SW)), 0
    for m, d in zip(cams, more):
        alone = R.seen(pts, m, K, SH, SW, d, 0.02)
        assert np.array_equal(device_seen(pts, [m], [d], 0.02), alone)
        before = int(want.sum())
        want = R.seen(pts, m, K, SH, SW, d, 0.02, out=want)
        plain = R.seen(pts, m, K, SH, SW, out=plain)
        grew += int(want.sum()) > before
    assert grew >= 2 and (want >= both).all() and want.sum() < 300
    assert np.array_equal(device_seen(pts, [np.eye(4), tilted] + cams, depths + more, 0.02), want)
    assert np.array_equal(device_seen(pts, [np.eye(4), tilted] + cams), plain)


# ---- metrics ------------------------------------------------------------------------------------------------------------------------------
def close(got, want):
    return abs(float(got) - float(want)) <= 1e-12 * abs(float(want))


def pieces(rec, gt, n, seed):
    """what mesh_metrics does, step by step: the samples of both sides and the two searches"""
    from hsr_utils import mesh_eval
    pr, _f, lr = mesh_eval.sample_mesh(*[dev(a) for a in rec[:2]], n, seed, None if len(rec) < 3 else dev(rec[2]))
    pg, _f, lg = mesh_eval.sample_mesh(*[dev(a) for a in gt[:2]], n, seed + 1, None if len(gt) < 3 else dev(gt[2]))
    area = lambda m: float(R.areas(*m[:2]).astype(np.float64).sum())
    d2_rec, _ = mesh_eval.NearestGrid(pg, 2.0 * np.sqrt(area(gt) / n)).query(pr)
    d2_gt, nearest = mesh_eval.NearestGrid(pr, 2.0 * np.sqrt(area(rec) / n)).query(pg)
    return pr, pg, lr, lg, d2_rec, d2_gt, nearest


def test_two_unit_squares_three_centimetres_apart():
    """accuracy and completion lie between the gap and the figures of the restatement, 0.03128 and 0.03126, plus 1 %; here, with the
    squares as 4 x 4 quads, the restatement gives 0.031254 and 0.031242"""
    from hsr_utils import mesh_eval
    rec, gt = R.unit_square(0.0), R.unit_square(0.03)
    got = mesh_eval.mesh_metrics(tuple(dev(a) for a in rec), tuple(dev(a) for a in gt), n_samples=4096, threshold=0.05, seed=0)
    pr, pg, _lr, _lg, d2_rec, d2_gt, _nearest = pieces(rec, gt, 4096, 0)
    want_d2 = R.brute_nn(pr.cpu().numpy(), pg.cpu().numpy())[0], R.brute_nn(pg.cpu().numpy(), pr.cpu().numpy())[0]
    assert np.array_equal(bits(d2_rec), bits(want_d2[0])) and np.array_equal(bits(d2_gt), bits(want_d2[1]))
    want = R.metrics(want_d2[0], want_d2[1], 0.05)
    assert set(got) == set(want)
    for name in want:
        print("%s: %.9f (restatement %.9f)" % (name, float(got[name]), want[name]))
        assert got[name].dtype == torch.float64 and got[name].dim() == 0 and got[name].is_cuda and close(got[name], want[name]), name
    assert 0.03 <= float(got["accuracy"]) < 0.03128 * 1.01 and 0.03 <= float(got["completion"]) < 0.03126 * 1.01
    assert float(got["completion_ratio"]) == 1.0 and float(got["accuracy_ratio"]) == 1.0 and float(got["f_score"]) == 1.0
    tight = mesh_eval.mesh_metrics(tuple(dev(a) for a in rec), tuple(dev(a) for a in gt), n_samples=4096, threshold=0.031, seed=0)
    want_tight = R.metrics(want_d2[0], want_d2[1], 0.031)
    assert 0 < want_tight["completion_ratio"] < 1 and all(close(tight[name], want_tight[name]) for name in want_tight)
    far = mesh_eval.mesh_metrics(tuple(dev(a) for a in rec), tuple(dev(a) for a in gt), n_samples=4096, threshold=0.02, seed=0)
    assert float(far["accuracy_ratio"]) == 0 and float(far["completion_ratio"]) == 0 and float(far["f_score"]) == 0      # not a NaN


def test_a_mesh_against_itself_with_equal_seeds():
    from hsr_utils import mesh_eval
    vertices, faces = R.unit_square(0.0)
    labels = (vertices[:, 0] > 0.5).astype(np.int32)
    a = mesh_eval.sample_mesh(dev(vertices), dev(faces), 3000, 5, dev(labels))
    b = mesh_eval.sample_mesh(dev(vertices), dev(faces), 3000, 5, dev(labels))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    d2, nearest = mesh_eval.NearestGrid(a[0], 0.04).query(b[0])
    assert (d2 == 0).all()
    assert torch.equal(a[0][nearest.long()], b[0])      # the smallest index of a point at distance 0: the point itself or an equal one
    m = mesh_eval.distance_metrics(d2, d2, 0.05)
    assert [float(m[n]) for n in ("accuracy", "completion", "chamfer")] == [0, 0, 0]
    assert [float(m[n]) for n in ("accuracy_ratio", "completion_ratio", "f_score")] == [1, 1, 1]
    lab = mesh_eval.label_metrics(b[2], a[2], nearest, 2)
    assert float(lab["miou"]) == 1 and float(lab["label_accuracy"]) == 1 and lab["confusion"].tolist() == [[int((a[2] == 0).sum()), 0], [0, int((a[2] == 1).sum())]]


def test_label_confusion_equals_the_restatement():
    """left half 0, right half 1; a strip of the ground truth relabelled, one vertex column ignored (-1)"""
    from hsr_utils import mesh_eval
    rv, rf = R.unit_square(0.0, n=8)
    gv, gf = R.unit_square(0.01, n=8)
    rl = (rv[:, 0] > 0.5).astype(np.int32)
    gl = (gv[:, 0] > 0.5).astype(np.int32)
    gl[(gv[:, 0] > 0.2) & (gv[:, 0] < 0.4)] = 1      # the strip
    gl[gv[:, 0] == 1.0] = -1
    n = 4096
    got = mesh_eval.mesh_metrics((dev(rv), dev(rf), dev(rl)), (dev(gv), dev(gf), dev(gl)), n_samples=n, threshold=0.05, seed=2, num_classes=2)
    _pr, _pg, lr, lg, d2_rec, d2_gt, nearest = pieces((rv, rf, rl), (gv, gf, gl), n, 2)
    want = R.metrics(d2_rec.cpu().numpy(), d2_gt.cpu().numpy(), 0.05, lg.cpu().numpy(), lr.cpu().numpy(), nearest.cpu().numpy(), 2)
    assert got["confusion"].dtype == torch.int64 and got["confusion"].tolist() == want["confusion"].tolist()
    assert want["confusion"][1, 0] > 100 and want["confusion"][0, 1] < want["confusion"][1, 0] and want["confusion"].sum() < n
    assert close(got["label_accuracy"], want["label_accuracy"]) and close(got["miou"], want["miou"]) and 0.5 < want["miou"] < 0.95
    # without num_classes: one more than the largest label; labels on one side only: no label numbers
    auto = mesh_eval.mesh_metrics((dev(rv), dev(rf), dev(rl)), (dev(gv), dev(gf), dev(gl)), n_samples=n, threshold=0.05, seed=2)
    assert auto["confusion"].tolist() == want["confusion"].tolist()
    assert "miou" not in mesh_eval.mesh_metrics((dev(rv), dev(rf)), (dev(gv), dev(gf), dev(gl)), n_samples=64)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
VOXEL, EVERY = 0.08, 2
SCORE = dict(voxel_size=VOXEL, every=EVERY, threshold=2 * VOXEL, n_samples=20000)


@pytest.fixture(scope="module")
def session(sequence):  # noqa: F811
    """the short session of tests/test_gpu_mesh_run.py (2 tracking and 2 mapping iterations a frame), built afresh"""
    from hsr_utils import SlamSession
    cam, intrinsics, frames = sequence
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    config = TS._config(2)
    config["mapping"]["num_iters"] = 2
    s = SlamSession(config, intrinsics, torch.eye(4, device="cuda"), cam)
    for frame in frames:
        s.step(frame)
    return s


def test_a_run_scored_against_its_own_mesh(session, tmp_path):
    from hsr_utils import mesh
    own = session.export_mesh(str(tmp_path / "own.ply"), voxel_size=VOXEL, every=EVERY)
    first = session.evaluate_mesh(own[0], **SCORE)
    again = session.evaluate_mesh(own[0], **SCORE)
    assert set(first) == set(again) and {"accuracy", "completion", "completion_ratio", "confusion", "miou", "gt_faces_kept"} <= set(first)
    for name in first:      # deterministic across two calls
        assert torch.equal(first[name], again[name]) if isinstance(first[name], torch.Tensor) else first[name] == again[name], name
    print({n: (float(v) if isinstance(v, torch.Tensor) and v.dim() == 0 else v) for n, v in first.items() if n != "confusion"})
    assert (first["rec_vertices"], first["rec_faces"]) == own[1:] == (first["gt_vertices"], first["gt_faces"])
    assert 0 < first["gt_faces_kept"] <= first["gt_faces"] and 0 < first["gt_vertices_seen"] <= first["gt_vertices"]
    assert float(first["completion_ratio"]) == 1.0      # at a threshold of two voxels
    assert 0 < float(first["completion"]) < VOXEL and 0 <= float(first["miou"]) <= 1 and 1 <= first["confusion"].shape[0] <= TS.K
    # ground-truth vertices behind the cameras (and their faces) are culled: the score is that of the mesh without them
    vertices, faces, rgb, labels = mesh.load_mesh_ply(own[0])
    behind = np.array([[0, 0, -2], [1, 0, -2], [0, 1, -2], [0.5, 0.5, -3]], np.float32)
    more_faces = np.array([[0, 1, 2], [1, 2, 3]], np.int32) + len(vertices)
    padded = mesh.save_mesh_ply(str(tmp_path / "padded.ply"), np.concatenate([vertices, behind]), np.concatenate([faces, more_faces]),
                                np.concatenate([rgb, np.zeros((4, 3), np.uint8)]), np.concatenate([labels, np.zeros(4, np.int32)]))
    culled = session.evaluate_mesh(padded, **SCORE)
    assert (culled["gt_vertices"], culled["gt_faces"]) == (len(vertices) + 4, len(faces) + 2)
    assert (culled["gt_vertices_seen"], culled["gt_faces_kept"]) == (first["gt_vertices_seen"], first["gt_faces_kept"])
    for name in ("accuracy", "completion", "completion_ratio", "f_score", "miou", "confusion"):
        assert torch.equal(culled[name], first[name]), name
    unculled = session.evaluate_mesh(padded, cull=False, **SCORE)
    assert unculled["gt_faces_kept"] == len(faces) + 2 and float(unculled["completion_ratio"]) < 1.0      # the faces behind the cameras count


def test_the_tool_in_a_fresh_process(session, sequence, tmp_path):  # noqa: F811
    from hsr_utils import map_io, mesh_eval
    s = session
    cam, intrinsics, frames = sequence
    out = map_io.finalize_params(s.params, s.variables, intrinsics, torch.eye(4), TS.W, TS.H, [f["gt_w2c"] for f in frames], s.keyframe_time_indices)
    saved = map_io.save_params(out, str(tmp_path / "run"))
    own = s.export_mesh(str(tmp_path / "own.ply"), voxel_size=VOXEL, every=EVERY)
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "eval_mesh.py")
    target = str(tmp_path / "score.json")
    done = subprocess.run([sys.executable, tool, saved, own[0], "--voxel-size", str(VOXEL), "--every", str(EVERY), "--threshold", str(2 * VOXEL),
                           "--samples", "20000", "--semantic", "--out", target], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    score = json.load(open(target))
    assert json.loads(done.stdout.strip().splitlines()[-1]) == score
    assert score["completion_ratio"] == 1.0 and 0 < score["completion"] < VOXEL and 0 < score["accuracy"] < VOXEL and 0 <= score["miou"] <= 1
    assert score["gt_faces"] == own[2] and 0 < score["gt_faces_kept"] <= own[2] and score["samples"] == 20000
    # the saved run through the module, with the file's own camera as the tool builds it: the tool's numbers
    params = map_io.load_params(saved, device="cuda")
    again = mesh_eval.evaluate_mesh_run(params, own[0], semantic=True, **SCORE)
    assert float(again["completion"]) == score["completion"] and float(again["accuracy"]) == score["accuracy"] and again["gt_faces_kept"] == score["gt_faces_kept"]
