"""CPU suite for the registration of a run's mesh (include/align/hsr_mesh_align.h, hsr_utils.mesh_align): the header through the helpers
of tests/test_abi.py (its prototypes, that the library exports them and that _abi.ALIGN_HEADERS binds them with the header's types);
every refusal of the header with dummy pointers; the scratch size; the lazy names; rigid_from_sums and trajectory_alignment against known
motions; the host errors; that evaluate_mesh_run and the tool carry the new keywords; and that the float64 reference ICP of
tests/mesh_align_ref.py alone recovers the displacement of the scene tests/test_gpu_mesh_align.py registers.  Nothing here launches:
there is no GPU."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import mesh_align_ref as R
import test_abi

HEADER = "align/hsr_mesh_align.h"
NAMES = ["hsr_icp_scratch_bytes", "hsr_icp_step"]
VP, IP, FP = ("pointer", "void"), ("pointer", "int"), ("pointer", "float")


# ---- the header ------------------------------------------------------------------------------------------------------------------------------
def test_mesh_align_abi_exported_and_bound():
    from diff_gaussian_rasterization import _abi
    protos = test_abi._prototypes([HEADER])
    assert list(_abi.ALIGN_HEADERS) == [HEADER] and HEADER not in test_abi.ALL_HEADERS
    others = (_abi.HEADERS, _abi.EVAL_HEADERS, _abi.RECON_HEADERS, _abi.SENSOR_HEADERS, _abi.SURFACE_HEADERS)
    assert all(HEADER not in table for table in others)
    assert [s[0] for s in _abi.ALIGN_HEADERS[HEADER]] == list(protos) == NAMES      # the header's names in the header's order
    assert test_abi.check_header(HEADER) == NAMES      # exported, and bound with the header's type classes
    for name, restype, argtypes in _abi.ALIGN_HEADERS[HEADER]:      # _load() bound this table as it binds the other five
        fn = getattr(_abi.lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    bound = [s[0] for tables in others + (_abi.ALIGN_HEADERS,) for table in tables.values() for s in table]
    assert sorted(bound) == sorted(set(bound))      # no name twice across the six tables
    assert protos["hsr_icp_scratch_bytes"][1:] == ("size_t", ["int"])
    assert protos["hsr_icp_step"][1:] == ("int", ["int", "int", "int", "float", "float", "float", "float", "int", IP, VP, "int", FP, FP, "float",
                                                  IP, FP, ("pointer", "double"), VP, "size_t", VP])
    step = dict((s[0], s[2]) for s in _abi.ALIGN_HEADERS[HEADER])["hsr_icp_step"]
    assert step[12] is _abi.fp and step[11] is _abi.vp      # the transform is the one HOST array
    from hsr_utils import mesh_align
    assert "#define HSR_ICP_SUMS %d\n" % mesh_align.SUMS in test_abi._source(HEADER) and mesh_align.SUMS == R.SUMS == 17


def test_names_are_reached_lazily_from_the_package():
    import hsr_utils
    from hsr_utils import mesh_align, mesh_eval
    assert tuple(hsr_utils._MESH_ALIGN) == tuple(mesh_align.__all__)
    for name in hsr_utils._MESH_ALIGN:
        assert getattr(hsr_utils, name) is getattr(mesh_align, name), name
    taken = set(hsr_utils._MESH_CLEAN) | set(hsr_utils._MESH_DEPTH) | set(hsr_utils._MESH_EVAL) | set(hsr_utils._MESH)
    assert not set(hsr_utils._MESH_ALIGN) & taken
    keywords = inspect.signature(mesh_eval.evaluate_mesh_run).parameters      # every new keyword defaults to "off"
    assert [keywords[n].default for n in ("align", "align_max_dist", "align_iterations", "gt_w2cs")] == [None, 0.1, 30, None]
    defaults = inspect.signature(mesh_align.icp).parameters
    assert [defaults[n].default for n in ("max_dist", "init", "max_iterations", "relative_fitness", "relative_rmse", "cell")] \
        == [0.1, None, 30, 1e-6, 1e-6, None]
    tool = open(os.path.join(test_abi.ROOT, "tools", "eval_mesh.py")).read()
    assert all(option in tool for option in ('"--align"', '"--align-max-dist"', '"--align-iterations"', '"--gt-poses"'))


# ---- refusals: dummy non-device pointers that are never followed; the transform is a real host array, since it is read -------------------
D = [4096 * (n + 1) for n in range(8)]      # 16-byte aligned
IDENTITY = np.eye(4, dtype=np.float32)[:3].reshape(12).copy()


def step_call(lib, X=4, Y=4, Z=4, ox=0.0, oy=0.0, oz=0.0, c=0.1, M=10, cell_start=D[0], packed=D[1], N=5, source=D[2], transform=IDENTITY,
              max_dist=0.1, out_index=D[3], out_d2=D[4], out_sums=D[5], scratch=D[6], scratch_bytes=None):
    from diff_gaussian_rasterization import _abi
    if scratch_bytes is None:
        scratch_bytes = lib.hsr_icp_scratch_bytes(max(N, 0))
    host = None if transform is None else np.ascontiguousarray(transform, np.float32).ctypes.data_as(_abi.fp)
    return lib.hsr_icp_step(X, Y, Z, ox, oy, oz, c, M, cell_start, packed, N, source, host, max_dist, out_index, out_d2, out_sums, scratch,
                            scratch_bytes, None)


def bad_transform(at, value):
    m = IDENTITY.copy()
    m[at] = value
    return m


NAN, INF = float("nan"), float("inf")
REFUSALS = (
    # what hsr_nn_query refuses
    [(o, b"invalid grid") for o in (dict(X=0), dict(Y=-1), dict(Z=1025), dict(X=1024, Y=1024, Z=17))]
    + [(o, b"the cell size must be finite and positive and the origin finite") for o in (dict(c=0.0), dict(c=-1.0), dict(c=NAN), dict(c=INF),
                                                                                         dict(ox=NAN), dict(oy=INF), dict(oz=-INF))]
    + [(o, b"invalid sizes") for o in (dict(N=-1), dict(M=0), dict(M=-4))]
    + [({n: None}, b"cell_start, packed and source are required with N > 0") for n in ("cell_start", "packed", "source")]
    + [(dict(packed=D[1] + 8), b"packed must be 16-byte aligned"), (dict(packed=D[1] + 4), b"packed must be 16-byte aligned")]
    # and its own
    + [(dict(transform=None), b"transform (12 floats on the host) is required")]
    + [(dict(transform=bad_transform(at, v)), b"transform entry %d is not finite" % at) for at, v in ((0, NAN), (3, INF), (7, -INF), (11, NAN))]
    + [(dict(max_dist=v), b"max_dist must be finite and positive") for v in (0.0, -0.1, NAN, INF)]
    + [(dict(out_sums=None), b"out_sums (17 float64) is required")]
    + [(dict(out_index=None), b"out_index and out_d2 come together"), (dict(out_d2=None), b"out_index and out_d2 come together")]
    + [(dict(scratch=None), b"the scratch must hold"), (dict(scratch_bytes=0), b"the scratch must hold"),
       (dict(scratch_bytes=17 * 8 - 1), b"the scratch must hold"), (dict(N=257, scratch_bytes=17 * 8), b"the scratch must hold"),
       (dict(scratch=D[6] + 4), b"8-byte aligned")]
)


@pytest.mark.parametrize("overrides,message", REFUSALS, ids=["%d" % i for i in range(len(REFUSALS))])
def test_icp_step_refuses_before_any_device_work(overrides, message):
    from diff_gaussian_rasterization import _abi
    rc = step_call(_abi.lib, **overrides)
    err = _abi.lib.hsr_last_error()
    assert rc == -1 and err.startswith(b"icp_step: ") and message in err, (overrides, rc, err)


def test_scratch_bytes_is_zero_without_points_and_does_not_decrease():
    from diff_gaussian_rasterization import _abi
    size = _abi.lib.hsr_icp_scratch_bytes
    assert size(0) == 0 and size(-1) == 0 and size(-2 ** 31) == 0
    assert size(1) == size(256) == 17 * 8 and size(257) == 2 * 17 * 8      # a row of 17 float64 per 256 points
    sizes = [size(n) for n in (0, 1, 255, 256, 257, 1000, 200000, 10 ** 7, 2 ** 31 - 1)]
    assert sizes == sorted(sizes) and all(s % 8 == 0 for s in sizes) and sizes[-1] == 17 * 8 * 2 ** 23


# ---- the closed form ------------------------------------------------------------------------------------------------------------------------
def known_motion(seed):
    g = np.random.default_rng(seed)
    rot = R.rotation(g.standard_normal(3), g.uniform(5, 170))
    return rot, g.standard_normal(3)


@pytest.mark.parametrize("seed", range(4))
def test_rigid_from_sums_recovers_a_known_motion(seed):
    from hsr_utils import mesh_align
    g = np.random.default_rng(100 + seed)
    rot, shift = known_motion(seed)
    p = g.standard_normal((50, 3)) * [1.0, 2.0, 0.5] + [3.0, -1.0, 2.0]
    q = p @ rot.T + shift
    sums = R.sums_of(p, q)
    got_r, got_t = mesh_align.rigid_from_sums(sums)
    assert got_r.dtype == got_t.dtype == np.float64 and got_r.shape == (3, 3) and got_t.shape == (3,)
    assert np.abs(got_r - rot).max() <= 1e-12 and np.abs(got_t - shift).max() <= 1e-12
    want_r, want_t = R.rigid_from_sums(sums)
    assert np.abs(got_r - want_r).max() <= 1e-15 and np.abs(got_t - want_t).max() <= 1e-15
    again = mesh_align.rigid_from_sums(torch.as_tensor(sums))      # a tensor, as icp_step returns it
    assert np.array_equal(again[0], got_r) and np.array_equal(again[1], got_t)
    # the closed form of evaluate._align, which trajectory_ate uses, from the points themselves
    from hsr_utils.evaluate import _align
    align_r, align_t, _err = _align(p.T, q.T)
    assert np.abs(got_r - align_r).max() <= 1e-12 and np.abs(got_t - align_t.reshape(3)).max() <= 1e-12


def test_rigid_from_sums_takes_the_reflection_branch_on_a_planar_set():
    """points in a plane: the third singular value is 0 and the SVD is free to return a reflection; the determinant's sign on the last
    singular direction must turn it into the rotation.  Over many motions both branches are taken."""
    from hsr_utils import mesh_align
    g = np.random.default_rng(5)
    branches = set()
    for seed in range(24):
        rot, shift = known_motion(50 + seed)
        p = np.concatenate([g.standard_normal((40, 2)), np.zeros((40, 1))], axis=1)      # z = 0
        q = p @ rot.T + shift
        sums = R.sums_of(p, q)
        n, mp, mq = sums[0], sums[1:4] / sums[0], sums[4:7] / sums[0]
        U, _d, Vh = np.linalg.svd((sums[7:16].reshape(3, 3) - n * np.outer(mp, mq)).T)
        branches.add(bool(np.linalg.det(U) * np.linalg.det(Vh) < 0))
        got_r, got_t = mesh_align.rigid_from_sums(sums)
        assert abs(np.linalg.det(got_r) - 1) <= 1e-12      # a rotation, never a reflection
        assert np.abs(got_r - rot).max() <= 1e-12 and np.abs(got_t - shift).max() <= 1e-12, seed
    assert branches == {False, True}


def test_rigid_from_sums_raises_below_three_points():
    from hsr_utils import mesh_align
    p = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    for n in (0, 1, 2):
        with pytest.raises(ValueError, match="a rigid motion needs three"):
            mesh_align.rigid_from_sums(R.sums_of(p[:n], p[:n]) if n else np.zeros(17))
    mesh_align.rigid_from_sums(R.sums_of(p, p))      # three are enough
    with pytest.raises(RuntimeError, match="sums must hold 17 numbers"):
        mesh_align.rigid_from_sums(np.zeros(16))


# ---- the trajectory --------------------------------------------------------------------------------------------------------------------------
def poses(n, seed):
    """n world-to-camera matrices with centres on a bent path"""
    g = np.random.default_rng(seed)
    out = []
    for i in range(n):
        c2w = np.eye(4)
        c2w[:3, :3] = R.rotation(g.standard_normal(3), g.uniform(0, 60))
        c2w[:3, 3] = [0.2 * i, 0.5 * np.sin(0.4 * i), 0.03 * i * i]
        out.append(np.linalg.inv(c2w))
    return np.stack(out)


def test_trajectory_alignment_recovers_a_known_world_change():
    from hsr_utils import mesh_align
    est = poses(20, 1)
    change = np.eye(4)      # the estimate's world -> the ground truth's
    change[:3, :3], change[:3, 3] = known_motion(9)
    gt = np.stack([m @ np.linalg.inv(change) for m in est])      # the same cameras, seen from the other world
    got = mesh_align.trajectory_alignment(gt, est)
    assert got.dtype == np.float64 and got.shape == (4, 4) and np.abs(got - change).max() <= 1e-12
    assert np.abs(got - R.trajectory_alignment(gt, est)).max() <= 1e-12
    # a frame without a ground-truth pose is skipped, whatever the estimate says there; tensors and a longer ground truth are taken
    holed, wild = gt.copy(), est.copy()
    holed[7, 1, 2] = np.nan
    wild[7, :3, 3] += 100.0
    assert np.abs(mesh_align.trajectory_alignment(holed, wild) - change).max() <= 1e-12
    assert np.abs(mesh_align.trajectory_alignment(wild, wild)[:3, :3] - np.eye(3)).max() <= 1e-12
    assert np.abs(mesh_align.trajectory_alignment(gt, wild) - change).max() > 1e-3      # unless it counts
    more = np.concatenate([gt, poses(3, 2)])
    assert np.abs(mesh_align.trajectory_alignment(torch.as_tensor(more), [torch.as_tensor(m) for m in est]) - change).max() <= 1e-12
    # the [:3,3] columns that trajectory_ate aligns are another alignment: it does not map the worlds
    from hsr_utils.evaluate import _align
    rot, trans, _err = _align(est[:, :3, 3].T, gt[:, :3, 3].T)
    assert np.abs(rot - change[:3, :3]).max() > 1e-2
    with pytest.raises(ValueError, match="a rigid motion needs three"):
        mesh_align.trajectory_alignment(gt[:2], est[:2])
    with pytest.raises(RuntimeError, match="estimated poses for"):
        mesh_align.trajectory_alignment(gt[:5], est)


# ---- the host side -------------------------------------------------------------------------------------------------------------------------
def test_host_errors():
    from hsr_utils import mesh_align, mesh_eval
    p = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="grid must be a NearestGrid"):
        mesh_align.icp_step(p, p, np.eye(4), 0.1)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        mesh_align.transform_points(p, np.eye(4))
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        mesh_align.icp(p, p)
    with pytest.raises(ValueError, match="max_dist must be finite and positive"):
        mesh_align.icp(p, p, max_dist=0.0)
    with pytest.raises(ValueError, match="max_iterations must be >= 0"):
        mesh_align.icp(p, p, max_iterations=-1)
    with pytest.raises(RuntimeError, match=r"init must be \[4,4\] or \[3,4\]"):
        mesh_align.icp(p, p, init=np.eye(3))
    with pytest.raises(ValueError, match="init holds an entry that is not finite"):
        mesh_align.icp(p, p, init=np.full((4, 4), np.nan))
    with pytest.raises(ValueError, match="align must be None"):
        mesh_eval.evaluate_mesh_run({}, "none.ply", voxel_size=0.1, align="kabsch")
    with pytest.raises(ValueError, match="needs gt_w2cs"):
        mesh_eval.evaluate_mesh_run({}, "none.ply", voxel_size=0.1, align="trajectory")


# ---- the restatement, and the scene of the device suite ----------------------------------------------------------------------------------
def test_restatement_of_a_step():
    targets = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32)
    source = np.array([[0.5, 0, 0], [0.25, 0, 0], [0.75, 0, 0], [np.nan, 0, 0], [0, 1.0, 0], [5, 5, 5]], np.float32)
    shift = np.eye(4)
    shift[0, 3] = 0.25      # binary-exact: the moved points are 0.75, 0.5, 1.0, nan, (0.25, 1), far
    d2, index, sums, absolute = R.step(source, targets, shift, 0.5)
    assert index.tolist() == [1, 0, 1, -1, -1, -1]      # a tie at 0.5 goes to the smaller index, and so do the equal targets 1 and 2
    assert d2[:3].tolist() == [0.0625, 0.25, 0.0] and np.isinf(d2[3:]).all()      # exactly max_dist away is a correspondence
    assert sums[0] == 3 and sums[1] == 2.25 and sums[4] == 2.0 and sums[7] == 1.75 and sums[16] == 0.3125 and np.array_equal(sums, absolute)
    none = R.step(source, targets, shift, 1e-3)
    assert none[1].tolist() == [-1, -1, 1, -1, -1, -1] and none[2][0] == 1
    empty = R.step(source[:0], targets, shift, 0.5)
    assert empty[0].shape == (0,) and not empty[2].any()


def test_reference_icp_recovers_the_displacement_of_the_device_scene():
    """the condition tests/test_gpu_mesh_align.py relies on: from 3 degrees about a skew axis and 3 cm, with a correspondence distance of
    0.1 m, the float64 loop converges within 30 updates on 20 000 samples against an independent 20 000, every point keeps a
    correspondence, and the room's corners land within 5 mm of where they belong — a fifth of the samples' spacing of 28 mm.
    Measured 2026-10-21: 22 updates, 1.95 mm, inlier rmse 16.6 mm."""
    vertices, _faces = R.room()
    source, target = R.room_samples(20000, 11), R.room_samples(20000, 12)
    motion = R.displacement(3.0, 0.03)
    got = R.icp(R.apply64(source, motion).astype(np.float32), target, max_dist=0.1)
    error = R.transform_error(got["transform"], np.linalg.inv(motion), vertices)
    print("reference icp: %d updates, error %.3f mm, fitness %.5f, rmse %.3f mm" % (got["iterations"], 1e3 * error, got["fitness"], 1e3 * got["inlier_rmse"]))
    assert got["converged"] and got["iterations"] <= 30 and got["fitness"] == 1.0 and error <= 5e-3
    start = R.transform_error(np.eye(4), np.linalg.inv(motion), vertices)
    assert 0.05 < start < 0.1      # what there was to recover: more than ten times what is left
