"""GPU suite for the registration of a run's mesh (include/align/hsr_mesh_align.h, hsr_utils.mesh_align): a pass against the numpy
restatement of tests/mesh_align_ref.py — d2 and index bit for bit, the number exactly, every other sum within the bound of any order of
float64 addition — at the smallest sizes at which it can go wrong; two calls against each other; the loop end to end against the float64
reference loop on the same points; and evaluate_mesh_run with an alignment on the six-frame session of tests/test_gpu_mesh_eval.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_align_ref as R
import mesh_eval_ref as E
import test_gpu_slam_session as TS
from test_gpu_mesh_eval import EVERY, SCORE, VOXEL, session  # noqa: F401  (the fixture: the short session, built afresh for this module)
from test_gpu_slam_session import sequence  # noqa: F401  (the fixture under it)

pytestmark = pytest.mark.gpu

DEV = "cuda"


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    return t if dtype is None else t.to(dtype)


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- a step against the restatement ---------------------------------------------------------------------------------------------------------
FIXTURE = R.step_fixture()
NN = E.nn_fixtures()
SLIGHT = R.displacement(2.0, 0.02, middle=(0.5, 0.5, 0.5))      # for the unit-cube fixtures of the nearest-neighbour suite


def step_cases():
    """name -> (source, targets, cell, transform, max_dist)"""
    f, m = FIXTURE, FIXTURE["marks"]
    general = R.general_transform()
    cases = {"nn_" + name: (q, t, cell, SLIGHT, 0.15) for name, (q, t, cell) in NN.items()}
    cases["nn_uniform_identity"] = NN["uniform_c0.1"] + (np.eye(4), 0.05)
    cases["built_quarter_turn"] = (f["source"], f["targets"], f["cell"], f["transform"], f["max_dist"])
    cases["built_general"] = (f["source"], f["targets"], f["cell"], general, f["max_dist"])
    cases["one_cell_grid"] = (f["source"][m["bulk"]][:300] * np.float32(0.25), f["targets"][:50] * np.float32(0.25), 1.0, np.eye(4), 0.5)
    for n in (0, 1, 255, 256, 257):
        cases["N%d" % n] = (f["source"][m["bulk"]][:n], f["targets"], f["cell"], f["transform"], f["max_dist"])
    cases["no_correspondence"] = (f["source"][m["far"]], f["targets"], f["cell"], f["transform"], f["max_dist"])
    return cases


CASES = step_cases()
_WANT = {}


def want(name):
    """the restatement of a case, computed once and shared"""
    if name not in _WANT:
        source, targets, _cell, transform, max_dist = CASES[name]
        _WANT[name] = R.step(source, targets, transform, max_dist)
    return _WANT[name]


def device_step(name):
    from hsr_utils import mesh_align, mesh_eval
    source, targets, cell, transform, max_dist = CASES[name]
    grid = mesh_eval.NearestGrid(dev(targets), cell)
    src = dev(source).reshape(-1, 3)
    return grid, src, mesh_align.icp_step(grid, src, transform, max_dist, correspondences=True)


@pytest.mark.parametrize("name", list(CASES))
def test_a_step_equals_the_restatement(name):
    from hsr_utils import mesh_align
    source, targets, cell, transform, max_dist = CASES[name]
    grid, src, (sums, d2, index) = device_step(name)
    want_d2, want_index, want_sums, absolute = want(name)
    N = len(source)
    assert sums.dtype == torch.float64 and sums.shape == (17,) and d2.dtype == torch.float32 and index.dtype == torch.int32
    assert d2.shape == index.shape == (N,)
    assert np.array_equal(bits(d2), bits(want_d2)) and np.array_equal(index.cpu().numpy(), want_index)
    got = sums.cpu().numpy()
    assert got[0] == want_sums[0] == (want_index >= 0).sum()      # the number is exact
    bound = max(N - 1, 0) * 2.0 ** -53 * absolute      # holds for any order of float64 addition
    print("%s: N %d, correspondences %d, largest error over its bound %.3g" % (
        name, N, int(got[0]), max((abs(g - w) / b if b > 0 else float(g != w)) for g, w, b in zip(got, want_sums, bound))))
    assert (np.abs(got - want_sums) <= bound).all(), (got - want_sums, bound)
    # without the optional outputs: the same sums, byte for byte
    alone = mesh_align.icp_step(grid, src, transform, max_dist)
    assert torch.equal(alone, sums)
    # where there is a correspondence the answer is NearestGrid.query's on the transformed points
    moved = mesh_align.transform_points(src, transform)
    assert np.array_equal(bits(moved), bits(R.transform32(source, transform)))
    if N:
        q_d2, q_index = grid.query(moved)
        has = index >= 0
        assert torch.equal(d2[has], q_d2[has]) and torch.equal(index[has], q_index[has])
        m2 = np.float32(max_dist) * np.float32(max_dist)
        assert bool(((q_d2 <= float(m2)) & (q_index >= 0) == has).all())
    if name == "built_quarter_turn":
        m = FIXTURE["marks"]
        got_index, got_d2 = index.cpu().numpy(), d2.cpu().numpy()
        assert np.array_equal(bits(moved[torch.as_tensor(np.concatenate([m["exact"], m["above"]]), device=DEV)]),
                              bits(FIXTURE["arrived"][np.concatenate([m["exact"], m["above"]])]))      # they arrive where they were put
        assert got_d2[m["exact"]].tolist() == [0.25] and got_index[m["exact"]].tolist() == [2850]      # exactly max_dist: a correspondence
        assert np.isinf(got_d2[m["above"]]).all() and got_index[m["above"]].tolist() == [-1]           # one float above: none
        assert np.array_equal(got_index[m["twice"]], np.arange(100, 150))                               # of two equal targets, the first
        for part in ("nan", "outside", "far"):
            assert (got_index[m[part]] == -1).all() and np.isinf(got_d2[m[part]]).all(), part
        assert 0.5 < (got_index[m["bulk"]] >= 0).mean() < 1.0      # sources outside the box with and without a correspondence
    if name == "one_cell_grid":
        assert grid.dims == (1, 1, 1) and 0 < got[0] < N
    if name in ("no_correspondence", "N0"):
        assert not got.any() and (index == -1).all() and bool(torch.isinf(d2).all())      # 17 zeros


def test_two_calls_give_equal_bytes_and_the_order_of_the_points_does_not_matter():
    from hsr_utils import mesh_align
    source, _targets, _cell, transform, max_dist = CASES["built_general"]
    grid, src, (sums, d2, index) = device_step("built_general")
    again = mesh_align.icp_step(grid, src, transform, max_dist, correspondences=True)
    assert torch.equal(again[0].view(torch.int64), sums.view(torch.int64)) and torch.equal(again[1].view(torch.int32), d2.view(torch.int32))
    assert torch.equal(again[2], index)
    order = torch.as_tensor(np.random.default_rng(3).permutation(len(source)), device=DEV)
    shuffled = mesh_align.icp_step(grid, src[order].contiguous(), transform, max_dist, correspondences=True)
    assert shuffled[0][0] == sums[0] and torch.equal(shuffled[2], index[order]) and torch.equal(shuffled[1].view(torch.int32), d2[order].view(torch.int32))
    assert torch.equal(torch.sort(shuffled[2]).values, torch.sort(index).values)      # the same set of targets
    want_sums, absolute = want("built_general")[2:]
    assert (np.abs(shuffled[0].cpu().numpy() - want_sums) <= (len(source) - 1) * 2.0 ** -53 * absolute).all()


# ---- the loop ------------------------------------------------------------------------------------------------------------------------------
N_ICP = 20000
_ROOM = {}


def room_case():
    """the scene of the loop's test, made once and shared: N_ICP device samples of the room displaced by 3 degrees and 3 cm, an
    independent draw as the target, the float64 reference loop on the very same points, and the bound: ten times its error"""
    if not _ROOM:
        from hsr_utils import mesh_eval
        vertices, faces = R.room()
        source = mesh_eval.sample_mesh(dev(vertices), dev(faces), N_ICP, seed=11)[0].cpu().numpy()
        target = mesh_eval.sample_mesh(dev(vertices), dev(faces), N_ICP, seed=12)[0].cpu().numpy()
        motion = R.displacement(3.0, 0.03)
        moved = R.apply64(source, motion).astype(np.float32)
        reference = R.icp(moved, target, max_dist=0.1)
        error = R.transform_error(reference["transform"], np.linalg.inv(motion), vertices)
        _ROOM.update(vertices=vertices, moved=moved, target=target, motion=motion, reference=reference, error=error, bound=10 * error)
    return _ROOM


def test_icp_recovers_a_known_displacement():
    """3 degrees about a skew axis and 3 cm, 20 000 samples of the room of tests/mesh_align_ref.py against an independent 20 000: the
    farthest any vertex of the room lands from where the known motion's inverse puts it is held to ten times what the float64 reference
    loop leaves on the same points; the ten covers the float32 transform and the correspondences it flips near ties.  The reference's
    error, measured on the CPU 2026-10-21 with the restatement's samples: 1.95 mm after 22 updates (rmse 16.6 mm, fitness 1), so the
    bound is 19.5 mm against the 50 to 100 mm there are to recover."""
    from hsr_utils import mesh_align
    case = room_case()
    got = mesh_align.icp(dev(case["moved"]), dev(case["target"]), max_dist=0.1)
    assert got["transform"].dtype == np.float64 and got["transform"].shape == (4, 4)
    error = R.transform_error(got["transform"], np.linalg.inv(case["motion"]), case["vertices"])
    ref = case["reference"]
    print("device: %d updates, error %.3f mm, fitness %.5f, rmse %.3f mm; reference: %d updates, error %.3f mm, fitness %.5f, rmse %.3f mm" % (
        got["iterations"], 1e3 * error, got["fitness"], 1e3 * got["inlier_rmse"], ref["iterations"], 1e3 * case["error"], ref["fitness"],
        1e3 * ref["inlier_rmse"]))
    assert ref["converged"] and case["error"] < 5e-3      # the condition of tests/test_mesh_align_cpu.py, on these points
    assert error <= case["bound"]
    assert got["iterations"] <= 30 and got["converged"] is True and abs(got["fitness"] - ref["fitness"]) <= 1e-3
    assert np.abs(got["transform"][:3, :3] @ got["transform"][:3, :3].T - np.eye(3)).max() <= 1e-12 and got["transform"][3].tolist() == [0, 0, 0, 1]
    # a NearestGrid as the target, and a start that is the answer: no more than a pass or two
    from hsr_utils import mesh_eval
    grid = mesh_eval.NearestGrid(dev(case["target"]), 0.1)
    near = mesh_align.icp(dev(case["moved"]), grid, max_dist=0.1, init=got["transform"])
    assert near["converged"] and near["iterations"] <= 2
    capped = mesh_align.icp(dev(case["moved"]), grid, max_dist=0.1, max_iterations=3)
    assert capped["iterations"] == 3 and not capped["converged"]
    with pytest.raises(ValueError, match="a rigid motion needs three"):
        mesh_align.icp(dev(case["moved"] + np.float32(50)), grid, max_dist=0.1)


def test_align_mesh_moves_the_vertices_by_icp_of_surface_samples():
    from hsr_utils import mesh_align, mesh_eval
    vertices, faces = R.room()
    motion = R.displacement(3.0, 0.03)
    moved = R.apply64(vertices, motion).astype(np.float32)
    aligned, result = mesh_align.align_mesh((dev(moved), dev(faces)), (dev(vertices), dev(faces)), n_samples=N_ICP, seed=5)
    ps = mesh_eval.sample_mesh(dev(moved), dev(faces), N_ICP, 7)[0]
    pt = mesh_eval.sample_mesh(dev(vertices), dev(faces), N_ICP, 8)[0]
    same = mesh_align.icp(ps, pt)
    assert np.array_equal(same["transform"], result["transform"]) and same["iterations"] == result["iterations"]      # seed + 2 and seed + 3
    assert torch.equal(aligned, mesh_align.transform_points(dev(moved), result["transform"]))
    assert float((aligned - dev(vertices)).norm(dim=1).max()) <= room_case()["bound"] + 1e-5


# ---- a run -----------------------------------------------------------------------------------------------------------------------------------
TODAY = {"accuracy", "completion", "accuracy_ratio", "completion_ratio", "f_score", "chamfer", "confusion", "label_accuracy", "miou",
         "rec_vertices", "rec_faces", "gt_vertices", "gt_faces", "gt_vertices_seen", "gt_faces_kept"}


def test_a_run_aligned_to_its_own_displaced_mesh(session, tmp_path):  # noqa: F811
    from hsr_utils import mesh
    own = session.export_mesh(str(tmp_path / "own.ply"), voxel_size=VOXEL, every=EVERY)
    plain = session.evaluate_mesh(own[0], **SCORE)
    none = session.evaluate_mesh(own[0], align=None, **SCORE)
    assert set(plain) == set(none) == TODAY      # exactly today's keys
    for name in plain:
        assert torch.equal(plain[name], none[name]) if isinstance(plain[name], torch.Tensor) else plain[name] == none[name], name
    # the ground truth: the run's own mesh displaced by the motion of the loop's test, about the mesh's own middle
    vertices, faces, rgb, labels = mesh.load_mesh_ply(own[0])
    motion = R.displacement(3.0, 0.03, middle=np.asarray(vertices, np.float64).mean(axis=0))
    gt = mesh.save_mesh_ply(str(tmp_path / "displaced.ply"), R.apply64(vertices, motion).astype(np.float32), faces, rgb, labels)
    bound = room_case()["bound"]
    itself = float(plain["accuracy"])
    apart = session.evaluate_mesh(gt, depth_views=2, **SCORE)
    icp = session.evaluate_mesh(gt, align="icp", **SCORE)
    assert set(icp) == TODAY | {"align", "align_transform", "align_fitness", "align_rmse", "align_iterations"} and icp["align"] == "icp"
    error = R.transform_error(np.asarray(icp["align_transform"]), motion, vertices)
    print("accuracy: itself %.5f, displaced %.5f, after icp %.5f (bound %.5f); fitness %.4f, rmse %.5f, %d updates, transform error %.5f" % (
        itself, float(apart["accuracy"]), float(icp["accuracy"]), bound, icp["align_fitness"], icp["align_rmse"], icp["align_iterations"], error))
    assert float(apart["accuracy"]) > itself + bound      # there was something to align
    assert float(icp["accuracy"]) <= itself + bound and icp["align_fitness"] > 0.9
    assert np.asarray(icp["align_transform"]).shape == (4, 4) and 0 < icp["align_iterations"] <= 30 and 0 < icp["align_rmse"] < 0.1
    # the trajectory: ground-truth poses that are the run's own, seen from the displaced world; Depth L1 sees the aligned mesh too
    estimated = [m.detach().cpu().double().numpy() for m in session.estimated_w2c()]
    gt_w2cs = np.stack([m @ np.linalg.inv(motion) for m in estimated])
    with pytest.raises(ValueError, match="needs gt_w2cs"):
        session.evaluate_mesh(gt, align="trajectory", **SCORE)
    path = session.evaluate_mesh(gt, align="trajectory", gt_w2cs=gt_w2cs, depth_views=2, **SCORE)
    depth_keys = {"depth_l1", "depth_l1_covered", "depth_gt_cover", "depth_rec_cover", "depth_views"}
    assert set(path) == TODAY | depth_keys | {"align", "align_transform"} and path["align"] == "trajectory" and set(apart) == TODAY | depth_keys
    error = R.transform_error(np.asarray(path["align_transform"]), motion, vertices)
    print("after the trajectory's alignment: accuracy %.5f, transform error %.3g; depth L1 %.5f, displaced %.5f" % (
        float(path["accuracy"]), error, path["depth_l1"], apart["depth_l1"]))
    # the camera centres of six frames of a constant twist lie almost on a line: the turn about it is found from their sub-millimetre
    # spread, so the float32 poses' rounding shows in the transform — far inside the bound, which is all that is asked
    assert float(path["accuracy"]) <= itself + bound and error <= bound
    assert path["depth_l1"] < apart["depth_l1"]


def test_the_tool_aligns_in_a_fresh_process(session, sequence, tmp_path):  # noqa: F811
    from hsr_utils import map_io, mesh
    s = session
    _cam, intrinsics, frames = sequence
    out = map_io.finalize_params(s.params, s.variables, intrinsics, torch.eye(4), TS.W, TS.H, [f["gt_w2c"] for f in frames], s.keyframe_time_indices)
    saved = map_io.save_params(out, str(tmp_path / "run"))
    own = s.export_mesh(str(tmp_path / "own.ply"), voxel_size=VOXEL, every=EVERY)
    vertices, faces, rgb, labels = mesh.load_mesh_ply(own[0])
    motion = R.displacement(3.0, 0.03, middle=np.asarray(vertices, np.float64).mean(axis=0))
    gt = mesh.save_mesh_ply(str(tmp_path / "displaced.ply"), R.apply64(vertices, motion).astype(np.float32), faces, rgb, labels)
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "eval_mesh.py")
    target = str(tmp_path / "score.json")
    done = subprocess.run([sys.executable, tool, saved, gt, "--voxel-size", str(VOXEL), "--every", str(EVERY), "--threshold", str(2 * VOXEL),
                           "--samples", "20000", "--semantic", "--align", "icp", "--out", target], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    score = json.load(open(target))
    assert json.loads(done.stdout.strip().splitlines()[-1]) == score
    assert score["align"] == "icp" and np.asarray(score["align_transform"]).shape == (4, 4)
    assert score["align_fitness"] > 0.9 and 0 < score["align_rmse"] < 0.1 and 0 < score["align_iterations"] <= 30
    assert R.transform_error(np.asarray(score["align_transform"]), motion, vertices) < R.transform_error(np.eye(4), motion, vertices)
