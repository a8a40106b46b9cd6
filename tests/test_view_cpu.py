"""CPU suite for the novel-view path: the prototypes of include/ext/hsr_view.h (their names and type classes; tests/test_abi.py checks
that they are exported and bound with the header's types), every refusal of the header, the quaternion rule against build_rotation, the host
validity rule against torch's own expression, the Replica-V2 reader on a directory of tiny PNGs, and the argument errors of
render_view / evaluate_novel_views.  Nothing here launches: there is no GPU."""
import os

import numpy as np
import pytest
import torch

import test_abi
import view_ref as R

EXT_HEADER = "ext/hsr_view.h"
NAMES = ["hsr_view_prep", "hsr_view_holes_scratch_bytes", "hsr_view_holes"]


def test_view_abi_exported_and_bound():
    from diff_gaussian_rasterization import _abi
    protos = test_abi._prototypes([EXT_HEADER])
    assert [s[0] for s in _abi.HEADERS[EXT_HEADER]] == list(protos) == NAMES
    assert protos["hsr_view_prep"][1] == "int" and protos["hsr_view_prep"][2] == ["int"] * 4 + [("pointer", "float")] * 10 + [("pointer", "void")]
    assert protos["hsr_view_holes_scratch_bytes"][1:] == ("size_t", ["int", "int"])
    assert protos["hsr_view_holes"][2] == ["int", "int", ("pointer", "float"), ("pointer", "float"), "float", ("pointer", "int64_t"),
                                           ("pointer", "char"), "size_t", ("pointer", "void")]
    from hsr_utils import slam_helpers
    src = test_abi._source("hsr_frame_prep.h")
    assert "#define HSR_PREP_ROT_PARAMS 0" in src and "#define HSR_PREP_ROT_TRANSFORMED 1" in src
    assert (slam_helpers.ROT_PARAMS, slam_helpers.ROT_TRANSFORMED) == (R.ROT_PARAMS, R.ROT_TRANSFORMED) == (0, 1)


def test_names_are_reached_lazily_from_the_package():
    import hsr_utils
    from hsr_utils import evaluate, sequence, slam, slam_helpers
    assert hsr_utils.render_view is slam.render_view and hsr_utils.ReplicaV2Sequence is sequence.ReplicaV2Sequence
    assert hasattr(hsr_utils.SlamSession, "render_view") and callable(slam_helpers.transform_to_view)
    for name in ("view_holes", "view_percent_holes", "evaluate_novel_views"):
        assert name in evaluate.__all__ and callable(getattr(evaluate, name))


# ---- refusals: dummy non-device pointers that are never followed -------------------------------------------------------------------------
PREP_POINTERS = ("means3D", "unnorm_rotations", "logit_opacities", "log_scales", "w2c", "out_means3D", "out_unnorm_rot", "out_rotations",
                 "out_opacities", "out_scales")


def view_prep_call(lib, P=8, S=1, transform_rots=0, rot_source=0, **pointers):
    args = {name: 4096 * (k + 1) for k, name in enumerate(PREP_POINTERS)}
    args.update(pointers)
    return lib.hsr_view_prep(P, S, transform_rots, rot_source, *[args[n] for n in PREP_POINTERS], None)


PREP_REFUSALS = (
    [(dict(P=-1), b"invalid sizes P=-1"), (dict(P=-2 ** 31), b"invalid sizes")]
    + [(dict(S=s), b"log_scales must be [P,1] or [P,3]") for s in (0, 2, 4, -1)]
    + [(dict(rot_source=r), b"rot_source must be") for r in (2, -1)]
    + [(dict(w2c=None), b"w2c is required"), (dict(P=0, w2c=None), b"w2c is required")]
    + [({name: None}, b"are required") for name in ("means3D", "unnorm_rotations", "logit_opacities", "log_scales")]
    + [({name: None}, b"an output pointer is NULL") for name in ("out_means3D", "out_rotations", "out_opacities", "out_scales")]
)


@pytest.mark.parametrize("overrides,message", PREP_REFUSALS, ids=["%d" % i for i in range(len(PREP_REFUSALS))])
def test_view_prep_refuses_before_any_device_work(overrides, message):
    from diff_gaussian_rasterization import _abi
    rc = view_prep_call(_abi.lib, **overrides)
    err = _abi.lib.hsr_last_error()
    assert rc == -1 and err.startswith(b"view_prep: ") and message in err, (overrides, rc, err)


def test_an_empty_map_launches_nothing():
    """P = 0 succeeds with the NULL pointers of empty arrays (the matrix is still required), for both S and both rot sources"""
    from diff_gaussian_rasterization import _abi
    null = {name: None for name in PREP_POINTERS if name != "w2c"}
    for S in (1, 3):
        for rot_source in (0, 1):
            assert view_prep_call(_abi.lib, P=0, S=S, transform_rots=int(S == 3), rot_source=rot_source, **null) == 0
    assert view_prep_call(_abi.lib, P=0, S=2, **null) == -1


HOLES_REFUSALS = [
    (dict(H=0), b"invalid size H=0 W=7"), (dict(W=0), b"invalid size H=5 W=0"), (dict(H=-3), b"invalid size"), (dict(W=-1), b"invalid size"),
    (dict(H=65536, W=65536), b"invalid size"),
    (dict(silhouette=None), b"NULL silhouette"), (dict(gt_depth=None), b"NULL silhouette / gt_depth"), (dict(out2=None), b"out2"),
    (dict(scratch=None), b"scratch too small"), (dict(scratch_bytes=255), b"scratch too small: 256 bytes needed, 255 given"),
    (dict(scratch_bytes=0), b"scratch too small"), (dict(scratch=4098), b"not 4-byte aligned"),
    (dict(H=300, W=421, scratch_bytes=512), b"scratch too small: 768 bytes needed, 512 given"),
]


@pytest.mark.parametrize("overrides,message", HOLES_REFUSALS, ids=["%d" % i for i in range(len(HOLES_REFUSALS))])
def test_view_holes_refuses_before_any_device_work(overrides, message):
    from diff_gaussian_rasterization import _abi
    kw = dict(H=5, W=7, silhouette=4096, gt_depth=8192, sil_thres=0.5, out2=12288, scratch=16384, scratch_bytes=1 << 20)
    kw.update(overrides)
    rc = _abi.lib.hsr_view_holes(kw["H"], kw["W"], kw["silhouette"], kw["gt_depth"], kw["sil_thres"], kw["out2"], kw["scratch"],
                                 kw["scratch_bytes"], None)
    err = _abi.lib.hsr_last_error()
    assert rc == -1 and err.startswith(b"view_holes: ") and message in err, (overrides, rc, err)


def test_view_holes_scratch_bytes():
    from diff_gaussian_rasterization import _abi
    f = _abi.lib.hsr_view_holes_scratch_bytes
    # one pair of 32-bit counts per workgroup of 1024 pixels, at most 96 workgroups, rounded up to 256 bytes
    assert [f(1, 1), f(32, 32), f(32, 33), f(37, 53), f(300, 421), f(680, 1200), f(46340, 46340)] == [256, 256, 256, 256, 768, 768, 768]
    assert f(0, 5) > 0 and f(5, -1) > 0


# ---- the quaternion of a rotation matrix ------------------------------------------------------------------------------------------------
def _rot(axis, degrees):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    t = np.deg2rad(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


# (name, matrix, the pivot that decides): one per branch, a generic one with negative trace, and one with two equal pivots
ROTATIONS = [
    ("identity", np.eye(3), 0),
    ("half turn about x", np.diag([1.0, -1.0, -1.0]), 1),
    ("half turn about y", np.diag([-1.0, 1.0, -1.0]), 2),
    ("half turn about z", np.diag([-1.0, -1.0, 1.0]), 3),
    ("negative trace", _rot([0.3, -0.5, 0.81], 171.0), 3),
    ("tilted", _rot([0.9, 0.2, -0.1], 23.0), 0),
    ("two equal pivots", np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]]), 1),      # 180 degrees about (1, 1, 0): pivots 0, 2, 2, 0
]


@pytest.mark.parametrize("name,matrix,branch", ROTATIONS, ids=[r[0] for r in ROTATIONS])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_matrix_to_quaternion_then_build_rotation_returns_the_matrix(name, matrix, branch, dtype):
    from hsr_utils import slam
    build_rotation = R.build_rotation      # utils/slam_external.py:25-42, restated
    m = torch.tensor(matrix, dtype=dtype)
    pivots = [1 + m[0, 0] + m[1, 1] + m[2, 2], 1 + m[0, 0] - m[1, 1] - m[2, 2], 1 - m[0, 0] + m[1, 1] - m[2, 2], 1 - m[0, 0] - m[1, 1] + m[2, 2]]
    assert int(torch.stack(pivots).argmax()) == branch
    if name == "two equal pivots":
        assert pivots[1] == pivots[2] == 2
    q = slam.matrix_to_quaternion(m)
    assert q.shape == (4,) and q[0] >= 0 and abs(float(q.norm()) - 1) < 1e-6
    back = build_rotation(q[None])[0]
    assert float((back - m).abs().max()) <= 1e-6, (name, back, m)
    # the restatement the GPU suite compares the kernel with is the same rule
    assert torch.equal(R.matrix_to_quaternion(m), q)
    if dtype == torch.float32:      # and the package's own way from a pose column to a matrix takes the quaternion back as well
        pose = {"cam_unnorm_rots": q.reshape(1, 4, 1), "cam_trans": torch.zeros(1, 3, 1)}
        assert float((slam.frame_w2c(pose, 0)[:3, :3] - m).abs().max()) <= 1e-6
    assert torch.equal(slam.matrix_to_quaternion(m[None])[0], q)      # batched, as track_frame calls it


# ---- the validity rule -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numel", [1000, 2000, 3072, 7000, 37 * 53, 680 * 1200])
def test_validity_rule_equals_torchs_expression(numel):
    from hsr_utils.evaluate import view_percent_holes
    counts = [h for h in range(0, 2001) if h <= numel]
    mask = torch.ones(numel, dtype=torch.bool)
    want_pct, want_invalid = [], []
    for h in counts:      # ascending: one more False per step
        if h > 0:
            mask[h - 1] = False
        percent_holes = (~mask).sum() / mask.numel() * 100
        want_pct.append(percent_holes.item())
        want_invalid.append(bool(percent_holes > 0.1))
    pct, valid = view_percent_holes(np.asarray(counts), numel)
    assert pct.dtype == np.float32 and valid.dtype == np.bool_
    assert np.array_equal(pct, np.asarray(want_pct, np.float32)) and np.array_equal(valid, ~np.asarray(want_invalid))
    assert valid[0] and (numel < 2000 or not valid[min(2000, numel)])
    if numel % 1000 == 0:      # holes * 1000 == numel: 0.1 per cent in float32, which is not above float32(0.1): valid
        one, ok = view_percent_holes(numel // 1000, numel)
        assert ok and one == np.float32(0.1) and not view_percent_holes(numel // 1000 + 1, numel)[1]
    one, ok = view_percent_holes(3, 3072)
    assert one.shape == () and ok and not view_percent_holes(4, 3072)[1]


# ---- the Replica-V2 reader ---------------------------------------------------------------------------------------------------------------
def _pose(k):
    m = np.eye(4)
    m[:3, :3] = _rot([0.2 + 0.1 * k, 1.0, -0.3], 7.0 * k + 3.0)
    m[:3, 3] = (0.1 * k, -0.05 * k, 0.3 + 0.02 * k * k)
    return m


def _write_split(folder, n, first):
    """n frames of 8x6 PNGs whose pixel (0, 0) holds the frame's number, and traj_w_c.txt with the poses _pose(first + i)"""
    from PIL import Image
    os.makedirs(os.path.join(folder, "rgb"))
    os.makedirs(os.path.join(folder, "depth"))
    for i in range(n):
        rgb = np.full((6, 8, 3), 40, np.uint8)
        rgb[0, 0] = (first + i, i, 7)
        Image.fromarray(rgb).save(os.path.join(folder, "rgb", "rgb_%d.png" % i))
        depth = np.full((6, 8), 1000, np.uint16)
        depth[0, 0] = 100 * (first + i) + 1
        Image.fromarray(depth).save(os.path.join(folder, "depth", "depth_%d.png" % i))
    with open(os.path.join(folder, "traj_w_c.txt"), "w") as f:
        for i in range(n):
            f.write(" ".join(repr(float(v)) for v in _pose(first + i).reshape(-1)) + "\n")


@pytest.fixture()
def replica_v2(tmp_path):
    base = tmp_path / "data"
    _write_split(str(base / "room" / "imap" / "00"), 12, 0)
    _write_split(str(base / "room" / "imap" / "01"), 11, 50)
    return str(base)


def _rel(first, k):
    return np.linalg.inv(np.linalg.inv(_pose(first)) @ _pose(k)).astype(np.float32)


def test_replica_v2_both_splits(replica_v2):
    from hsr_utils import ReplicaSequence, ReplicaV2Sequence
    train = ReplicaV2Sequence(replica_v2, "room")
    assert isinstance(train, ReplicaSequence) and len(train) == 12 and train.use_train_split
    for i in (0, 1, 9, 10, 11):      # rgb_10 after rgb_9: the order of the numbers, not of the names
        color, depth, labels, w2c = train[i]
        assert color.dtype == np.uint8 and color.shape == (6, 8, 3) and depth.dtype == np.uint16 and depth.shape == (6, 8) and labels is None
        assert color[0, 0].tolist() == [i, i, 7] and depth[0, 0] == 100 * i + 1
        assert w2c.dtype == np.float32 and np.array_equal(w2c, _rel(0, i))
    assert np.allclose(train[0][3], np.eye(4), rtol=0, atol=1e-12)      # inverse(inverse(c2w_0) @ c2w_0) in float64
    test = ReplicaV2Sequence(replica_v2, "room", use_train_split=False)
    assert len(test) == 12 and not test.use_train_split and test.input_folder.endswith(os.path.join("imap", "01"))
    color, depth, labels, w2c = test[0]      # the first TRAINING frame, with the identity
    assert color[0, 0].tolist() == [0, 0, 7] and depth[0, 0] == 1 and labels is None and np.allclose(w2c, np.eye(4), rtol=0, atol=1e-12)
    for i in (1, 2, 10, 11):      # test view i - 1, relative to the first training frame
        color, depth, _labels, w2c = test[i]
        assert color[0, 0].tolist() == [50 + i - 1, i - 1, 7] and depth[0, 0] == 100 * (50 + i - 1) + 1
        assert np.array_equal(w2c, _rel(0, 50 + i - 1))
    assert [c[0, 0, 1] for c, _d, _l, _w in test][1:] == list(range(11))
    picked = ReplicaV2Sequence(replica_v2, "room", use_train_split=False, start=0, end=8, stride=3)
    assert picked.retained_inds == [0, 3, 6] and picked[1][0][0, 0].tolist() == [52, 2, 7] and np.array_equal(picked[2][3], _rel(0, 55))
    with pytest.raises(ValueError, match="stride"):
        ReplicaV2Sequence(replica_v2, "room", stride=0)


def test_replica_v2_errors(replica_v2):
    from hsr_utils import ReplicaV2Sequence
    os.remove(os.path.join(replica_v2, "room", "imap", "01", "depth", "depth_4.png"))
    with pytest.raises(RuntimeError, match="holds 11 rgb/rgb_\\*.png and 10 depth/depth_\\*.png"):
        ReplicaV2Sequence(replica_v2, "room", use_train_split=False)
    ReplicaV2Sequence(replica_v2, "room")      # the training split is whole
    traj = os.path.join(replica_v2, "room", "imap", "00", "traj_w_c.txt")
    lines = open(traj).read().splitlines()
    with open(traj, "w") as f:
        f.write("\n".join(lines[:11]) + "\n")
    with pytest.raises(RuntimeError, match="has 11 poses for 12 frames"):
        ReplicaV2Sequence(replica_v2, "room")
    with open(traj, "w") as f:
        f.write("\n".join([lines[0] + " 1.0"] + lines[1:]) + "\n")
    with pytest.raises(RuntimeError, match="line 1 has 17 numbers"):
        ReplicaV2Sequence(replica_v2, "room")
    with open(traj, "w") as f:
        f.write("\n")
    os.remove(os.path.join(replica_v2, "room", "imap", "01", "rgb", "rgb_4.png"))      # the test split's counts agree again
    with pytest.raises(RuntimeError, match="has 0 poses for 1 frames"):      # the first training pose is read for the test split
        ReplicaV2Sequence(replica_v2, "room", use_train_split=False)
    with pytest.raises(RuntimeError, match="holds 0 rgb"):
        ReplicaV2Sequence(replica_v2, "nowhere")


# ---- argument errors that need no device ---------------------------------------------------------------------------------------------------
def _host_params(P=5):
    g = torch.Generator().manual_seed(0)
    return {"means3D": torch.rand(P, 3, generator=g), "rgb_colors": torch.rand(P, 3, generator=g), "unnorm_rotations": torch.rand(P, 4, generator=g),
            "logit_opacities": torch.zeros(P, 1), "log_scales": torch.zeros(P, 1)}


def test_render_view_and_evaluate_novel_views_argument_errors():
    import hsr_utils
    from hsr_utils import evaluate, slam_helpers
    params = _host_params()
    for bad in (torch.zeros(3, 4), np.zeros((4, 4, 1)), torch.zeros(16), [[1.0, 0.0], [0.0, 1.0]]):
        with pytest.raises(RuntimeError, match=r"w2c must be \[4,4\] \(got \("):
            hsr_utils.render_view(params, bad, None, False)
        with pytest.raises(RuntimeError, match=r"w2c must be \[4,4\]"):
            slam_helpers.transform_to_view(params, bad)
    with pytest.raises(RuntimeError, match=r"got \(3, 4\)"):
        hsr_utils.render_view(params, torch.zeros(3, 4), None, True)
    with pytest.raises(RuntimeError, match="no CPU path"):      # a good matrix reaches the device check: host parameters are refused there
        hsr_utils.render_view(params, np.eye(4), None, False)
    frame = {"im": torch.zeros(3, 4, 4), "depth": torch.ones(1, 4, 4), "gt_w2c": torch.eye(4)}
    kw = dict(sil_thres=0.5, mapping_iters=1, add_new_gaussians=True)
    with pytest.raises(RuntimeError, match="save_frames needs eval_dir"):
        evaluate.evaluate_novel_views(params, [frame, frame], None, save_frames=True, **kw)
    for every in (0, -1):
        with pytest.raises(ValueError, match="eval_every must be >= 1"):
            evaluate.evaluate_novel_views(params, [frame, frame], None, eval_every=every, **kw)
    without = {k: v for k, v in frame.items() if k != "gt_w2c"}
    with pytest.raises(RuntimeError, match="novel view 0 carries no 'gt_w2c'"):      # the first item, the training frame, needs none
        evaluate.evaluate_novel_views(params, [without, without], None, **kw)
    with pytest.raises(RuntimeError, match=r"w2c must be \[4,4\] \(got \(3, 4\)\)"):
        evaluate.evaluate_novel_views(params, [without, dict(frame, gt_w2c=torch.zeros(3, 4))], None, **kw)
    with pytest.raises(RuntimeError, match="no view to score"):
        evaluate.evaluate_novel_views(params, [frame], None, **kw)
    with pytest.raises(RuntimeError, match="depth-plus-silhouette"):
        slam_helpers.transformed_params2depthplussilhouette(params, torch.eye(4), slam_helpers.transform_to_view(params, torch.eye(4)))
