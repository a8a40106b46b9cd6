"""CPU suite for the replay of a finished run: the prototypes of include/ext/hsr_replay.h (their names and type classes; tests/test_abi.py
checks that they are exported and bound with the header's types), every refusal of the header with dummy pointers, the empty map, the
scratch sizes, the pose and trajectory helpers against the reference's expressions, the lazy names and every host argument error.
Nothing here launches: there is no GPU."""
import os

import numpy as np
import pytest
import torch

import replay_ref as R
import test_abi

EXT_HEADER = "ext/hsr_replay.h"
NAMES = ["hsr_replay_plan_scratch_bytes", "hsr_replay_plan", "hsr_replay_select_scratch_bytes", "hsr_replay_select", "hsr_replay_cloud"]
FP, VP = ("pointer", "float"), ("pointer", "void")


def test_replay_abi_exported_and_bound():
    from diff_gaussian_rasterization import _abi
    protos = test_abi._prototypes([EXT_HEADER])
    assert [s[0] for s in _abi.HEADERS[EXT_HEADER]] == list(protos) == NAMES
    assert all(n.startswith("hsr_replay_") for n in NAMES)
    assert protos["hsr_replay_plan_scratch_bytes"][1:] == ("size_t", ["int", "int"])
    assert protos["hsr_replay_plan"][1:] == ("int", ["int", "int", FP, ("pointer", "int64_t"), ("pointer", "char"), "size_t", VP])
    assert protos["hsr_replay_select_scratch_bytes"][1:] == ("size_t", ["int"])
    assert protos["hsr_replay_select"][1:] == ("int", ["int"] * 7 + [FP] * 8 + [FP] * 7 + [("pointer", "int")] * 2 + [("pointer", "char"), "size_t", VP])
    assert protos["hsr_replay_cloud"][1:] == ("int", ["int", "int", FP, ("pointer", "uint8_t"), "float", "float", "float", "float", FP, FP,
                                                     ("pointer", "uint8_t"), VP])
    from hsr_utils import replay
    assert "#define HSR_REPLAY_MAX_STEPS (1 << 20)" in test_abi._source(EXT_HEADER) and replay.REPLAY_MAX_STEPS == 1 << 20


def test_names_are_reached_lazily_from_the_package():
    import hsr_utils
    from hsr_utils import replay
    assert set(hsr_utils._REPLAY) <= set(replay.__all__)
    for name in hsr_utils._REPLAY:
        assert getattr(hsr_utils, name) is getattr(replay, name), name
    assert callable(hsr_utils.SlamSession.replay)
    assert replay.CLOUD_FIELDS == (("float", "x"), ("float", "y"), ("float", "z"), ("uchar", "red"), ("uchar", "green"), ("uchar", "blue"))
    assert R.RECORD.names == tuple(n for _t, n in replay.CLOUD_FIELDS) and R.RECORD.itemsize == replay.CLOUD_RECORD_BYTES


# ---- refusals: dummy non-device pointers that are never followed -------------------------------------------------------------------------
def plan_call(lib, P=8, T=4, timestep=4096, out_upto=8192, scratch=16384, scratch_bytes=1 << 22):
    return lib.hsr_replay_plan(P, T, timestep, out_upto, scratch, scratch_bytes, None)


PLAN_REFUSALS = [
    (dict(P=-1), b"invalid sizes P=-1"), (dict(P=-2 ** 31), b"invalid sizes"), (dict(P=2 ** 31 - 1), b"invalid sizes"),
    (dict(T=0), b"invalid sizes P=8 T=0"), (dict(T=-5), b"invalid sizes"), (dict(T=(1 << 20) + 1), b"T in 1..1048576"),
    (dict(out_upto=None), b"NULL out_upto"), (dict(timestep=None), b"NULL timestep with P=8"),
    (dict(scratch=None), b"scratch too small"), (dict(scratch_bytes=255), b"scratch too small: 256 bytes needed, 255 given"),
    (dict(scratch_bytes=0), b"scratch too small"), (dict(scratch=16386), b"not 4-byte aligned"),
    (dict(T=1000, scratch_bytes=4095), b"scratch too small: 4096 bytes needed, 4095 given"),
]


@pytest.mark.parametrize("overrides,message", PLAN_REFUSALS, ids=["%d" % i for i in range(len(PLAN_REFUSALS))])
def test_replay_plan_refuses_before_any_device_work(overrides, message):
    from diff_gaussian_rasterization import _abi
    rc = plan_call(_abi.lib, **overrides)
    err = _abi.lib.hsr_last_error()
    assert rc == -1 and err.startswith(b"replay_plan: ") and message in err, (overrides, rc, err)


SELECT_IN = ("timestep", "means3D", "unnorm_rotations", "logit_opacities", "log_scales", "rgb_colors", "semantic", "w2c")
SELECT_OUT = ("out_means3D", "out_unnorm_rot", "out_rotations", "out_opacities", "out_scales", "out_colors", "out_semantic", "out_index",
              "out_count")


def select_call(lib, P=8, S=1, K=3, transform_rots=0, rot_source=0, step=2, capacity=8, scratch=1 << 20, scratch_bytes=1 << 16, **pointers):
    args = {name: 4096 * (k + 1) for k, name in enumerate(SELECT_IN + SELECT_OUT)}
    args.update(pointers)
    return lib.hsr_replay_select(P, S, K, transform_rots, rot_source, step, capacity, *[args[n] for n in SELECT_IN + SELECT_OUT], scratch,
                                 scratch_bytes, None)


SELECT_REFUSALS = (
    [(dict(P=-1), b"invalid sizes P=-1"), (dict(P=2 ** 31 - 1), b"invalid sizes"), (dict(K=-1), b"invalid sizes P=8 S=1 K=-1"),
     (dict(P=0, S=2), b"invalid sizes P=0 S=2"),      # an empty map is checked like any other (its success launches: tests/test_gpu_replay.py)
     (dict(K=1 << 23), b"invalid sizes")]
    + [(dict(S=s), b"log_scales must be [P,1] or [P,3]") for s in (0, 2, 4, -1)]
    + [(dict(rot_source=r), b"rot_source must be") for r in (2, -1)]
    + [(dict(transform_rots=1, w2c=None), b"transform_rots needs w2c"), (dict(P=0, S=3, transform_rots=1, w2c=None), b"transform_rots needs w2c")]
    + [(dict(capacity=-1), b"capacity=-1"), (dict(out_count=None), b"out_count not NULL"), (dict(P=0, out_count=None), b"out_count not NULL")]
    + [({name: None}, b"are required") for name in ("timestep", "means3D", "unnorm_rotations", "logit_opacities", "log_scales", "rgb_colors",
                                                    "semantic")]
    + [({name: None}, b"an output pointer is NULL") for name in ("out_means3D", "out_rotations", "out_opacities", "out_scales", "out_colors")]
    + [(dict(scratch=None), b"scratch too small"), (dict(scratch_bytes=255), b"scratch too small: 256 bytes needed, 255 given"),
       (dict(scratch=(1 << 20) + 2), b"not 4-byte aligned"), (dict(P=70001, scratch_bytes=1024), b"scratch too small: 1280 bytes needed")]
)


@pytest.mark.parametrize("overrides,message", SELECT_REFUSALS, ids=["%d" % i for i in range(len(SELECT_REFUSALS))])
def test_replay_select_refuses_before_any_device_work(overrides, message):
    from diff_gaussian_rasterization import _abi
    rc = select_call(_abi.lib, **overrides)
    err = _abi.lib.hsr_last_error()
    assert rc == -1 and err.startswith(b"replay_select: ") and message in err, (overrides, rc, err)


def cloud_call(lib, H=5, W=7, depth=4096, picture=8192, fx=100.0, fy=90.0, cx=3.0, cy=2.0, c2w=12288, out_points=16384, out_records=20480):
    return lib.hsr_replay_cloud(H, W, depth, picture, fx, fy, cx, cy, c2w, out_points, out_records, None)


CLOUD_REFUSALS = [
    (dict(H=0), b"invalid size H=0 W=7"), (dict(W=0), b"invalid size H=5 W=0"), (dict(H=-3), b"invalid size"), (dict(H=65536, W=65536), b"invalid size"),
    (dict(depth=None), b"NULL depth"), (dict(c2w=None), b"NULL depth / c2w"),
    (dict(fx=0.0), b"fx and fy must be finite and not zero"), (dict(fy=-0.0), b"finite and not zero"), (dict(fx=float("inf")), b"finite"),
    (dict(fy=float("nan")), b"finite"), (dict(fx=float("-inf")), b"finite"),
    (dict(out_points=None, out_records=None), b"out_points or out_records is required"),
    (dict(picture=None), b"picture with out_records"), (dict(picture=None, out_points=None), b"picture with out_records"),
]


@pytest.mark.parametrize("overrides,message", CLOUD_REFUSALS, ids=["%d" % i for i in range(len(CLOUD_REFUSALS))])
def test_replay_cloud_refuses_before_any_device_work(overrides, message):
    from diff_gaussian_rasterization import _abi
    rc = cloud_call(_abi.lib, **overrides)
    err = _abi.lib.hsr_last_error()
    assert rc == -1 and err.startswith(b"replay_cloud: ") and message in err, (overrides, rc, err)


def test_scratch_sizes():
    from diff_gaussian_rasterization import _abi
    plan, select = _abi.lib.hsr_replay_plan_scratch_bytes, _abi.lib.hsr_replay_select_scratch_bytes
    # T 32-bit bins, rounded up to 256 bytes; P does not matter
    assert [plan(0, 1), plan(5, 64), plan(10 ** 6, 65), plan(7, 1000), plan(7, 1 << 20)] == [256, 256, 512, 4096, 4 << 20]
    assert plan(5, 0) > 0 and plan(5, (1 << 20) + 1) > 0
    # one 32-bit count per 256 rows, rounded up to 256 bytes
    assert [select(0), select(1), select(256 * 64), select(256 * 64 + 1), select(70001), select(300007)] == [256, 256, 256, 512, 1280, 4864]
    assert select(-1) > 0


# ---- the poses and the trajectory ------------------------------------------------------------------------------------------------------------
def _pose_params(T=6, seed=3):
    g = torch.Generator().manual_seed(seed)
    return {"cam_unnorm_rots": torch.randn(1, 4, T, generator=g), "cam_trans": torch.randn(1, 3, T, generator=g)}


def test_run_w2cs_equals_frame_w2c():
    from hsr_utils import replay, slam
    params = _pose_params()
    w2cs = replay.run_w2cs(params)
    assert w2cs.shape == (6, 4, 4) and w2cs.dtype == torch.float32
    for t in range(6):
        assert torch.equal(w2cs[t], slam.frame_w2c(params, t)), t
        assert torch.equal(w2cs[t, 3], torch.tensor([0.0, 0.0, 0.0, 1.0]))
        assert float((w2cs[t, :3, :3] @ w2cs[t, :3, :3].T - torch.eye(3)).abs().max()) < 1e-5


def test_follow_camera_centres_and_lines_equal_the_references_expressions():
    from hsr_utils import replay
    w2cs = replay.run_w2cs(_pose_params()).numpy()
    first_view = w2cs[0].copy()
    first_view[:3, 3] = first_view[:3, 3] + np.array([0, 0, 0.5], np.float32)      # :314
    for t in range(len(w2cs)):
        want = np.dot(first_view, w2cs[t])      # :375
        assert np.array_equal(replay.follow_camera(first_view, w2cs[t]), want)
        got = replay.follow_camera(torch.tensor(first_view), torch.tensor(w2cs[t]))
        assert isinstance(got, torch.Tensor) and np.allclose(got.numpy(), want, rtol=0, atol=1e-6)
    centres = replay.camera_centres(w2cs)
    assert centres.shape == (6, 3) and np.array_equal(centres, R.camera_centres(w2cs))
    assert np.array_equal(replay.camera_centres(torch.tensor(w2cs)), centres)
    for n in (1, 2, 7):
        lines = replay.trajectory_lines(n)
        assert lines.dtype == np.int32 and lines.shape == (n - 1, 2) and np.array_equal(lines, R.trajectory_lines(n))
    assert replay.trajectory_lines(3).tolist() == [[1, 0], [2, 1]]


# ---- argument errors that need no device ---------------------------------------------------------------------------------------------------
def _host_params(P=5, K=None):
    g = torch.Generator().manual_seed(0)
    p = {"means3D": torch.rand(P, 3, generator=g), "rgb_colors": torch.rand(P, 3, generator=g), "unnorm_rotations": torch.rand(P, 4, generator=g),
         "logit_opacities": torch.zeros(P, 1), "log_scales": torch.zeros(P, 1)}
    p.update(_pose_params(4))
    if K:
        p["semantic"] = torch.rand(P, K, generator=g)
    return p


def _hand_plan(P, T):
    """a plan made by hand: ReplayPlan's own constructor launches"""
    from hsr_utils import replay
    plan = replay.ReplayPlan.__new__(replay.ReplayPlan)
    plan.timestep, plan.counts, plan.num_frames = torch.zeros(P), np.full(T, P, np.int64), T
    return plan


def test_host_argument_errors(tmp_path):
    from hsr_utils import replay
    params = _host_params()
    eye = np.eye(4, dtype=np.float32)
    k = np.array([[50.0, 0, 8], [0, 50.0, 6], [0, 0, 1]])
    # no 'timestep'
    with pytest.raises(RuntimeError, match="carries no 'timestep'"):
        replay.replay_run(params, str(tmp_path / "a"))
    # a timestep length other than P
    with pytest.raises(RuntimeError, match="timestep has 4 entries, the map 5 Gaussians"):
        replay.replay_run(dict(params, timestep=torch.zeros(4)), str(tmp_path / "a"))
    with pytest.raises(RuntimeError, match="timestep has 7 entries, the map 5 Gaussians"):
        replay.replay_rendervars(params, _hand_plan(7, 4), 0, semantic=False)
    # a step outside the plan
    plan = _hand_plan(5, 4)
    for step in (-1, 4, 100):
        with pytest.raises(ValueError, match="step %d is outside the plan's 0..3" % step):
            replay.replay_rendervars(params, plan, step, semantic=False)
        with pytest.raises(ValueError, match="outside the plan"):
            replay.replay_view(params, plan, step, eye, k, 16, 12, semantic=False)
    with pytest.raises(ValueError, match="step 9 is outside the run's 0..3"):
        replay.replay_run(dict(params, timestep=torch.zeros(5), intrinsics=k, org_width=16, org_height=12), str(tmp_path / "a"), steps=[9])
    # semantic=True without params['semantic']
    with pytest.raises(RuntimeError, match=r"semantic=True needs params\['semantic'\]"):
        replay.replay_rendervars(params, plan, 0, semantic=True)
    with pytest.raises(RuntimeError, match=r"semantic=True needs params\['semantic'\]"):
        replay.replay_view(params, plan, 0, eye, k, 16, 12, semantic=True)
    with pytest.raises(RuntimeError, match=r"semantic=True needs params\['semantic'\]"):
        replay.replay_run(dict(params, timestep=torch.zeros(5)), str(tmp_path / "a"), semantic=True)
    # records=True without a picture
    with pytest.raises(RuntimeError, match="records=True needs a picture"):
        replay.view_cloud(torch.zeros(1, 4, 4), k, eye, records=True)
    # a w2c that is not [4,4]
    for bad in (torch.zeros(3, 4), np.zeros((4, 4, 1)), torch.zeros(16), [[1.0, 0.0], [0.0, 1.0]]):
        with pytest.raises(RuntimeError, match=r"w2c must be \[4,4\] \(got \("):
            replay.replay_rendervars(params, plan, 0, semantic=False, w2c=bad)
        with pytest.raises(RuntimeError, match=r"w2c must be \[4,4\]"):
            replay.replay_view(params, plan, 0, bad, k, 16, 12, semantic=False)
        with pytest.raises(RuntimeError, match=r"w2c must be \[4,4\]"):
            replay.view_cloud(torch.zeros(1, 4, 4), k, bad)
        with pytest.raises(RuntimeError, match=r"w2c must be \[4,4\]"):
            replay.follow_camera(eye, bad)
        with pytest.raises(RuntimeError, match=r"w2c must be \[4,4\]"):
            replay.replay_run(dict(params, timestep=torch.zeros(5)), str(tmp_path / "a"), follow=bad)
    # the plan's own arguments, and host tensors where device ones are needed
    for frames in (0, -1, (1 << 20) + 1):
        with pytest.raises(ValueError, match="num_frames must be 1..1048576"):
            replay.ReplayPlan(torch.zeros(5), frames)
    with pytest.raises(RuntimeError, match="no CPU path"):
        replay.ReplayPlan(torch.zeros(5), 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        replay.replay_rendervars(params, plan, 0, semantic=False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        replay.view_cloud(torch.zeros(1, 4, 4), k, eye)
    for kw, message in ((dict(picture="normals"), "picture must be one of"), (dict(picture="semantic"), "needs semantic=True"), (dict(every=0), "every must be >= 1")):
        with pytest.raises(ValueError, match=message):
            replay.replay_run(dict(params, timestep=torch.zeros(5)), str(tmp_path / "a"), **kw)
    assert not os.path.exists(str(tmp_path / "a"))      # refused before anything was written
    from hsr_utils import slam
    session = slam.SlamSession.__new__(slam.SlamSession)
    session.params = None
    with pytest.raises(RuntimeError, match="replay before the first frame"):
        session.replay(str(tmp_path / "b"))
