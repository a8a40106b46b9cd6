"""CPU suite for the packed keyframe store and a session's checkpoint and resume: the prototypes of include/ext/hsr_keyframe_pack.h (their
names and type classes; tests/test_abi.py checks that they are exported and bound with the header's types), every refusal of the header with
dummy pointers, the scratch sizes, the exactness condition of the codes on the numpy restatement (all 256 grey levels and all 65 536
depth codes), the three config keys, and save_checkpoint / load_checkpoint on a hand-built host session whose keyframes stay as they
are.  Nothing here launches: there is no GPU."""
import os
import types

import numpy as np
import pytest
import torch

import keyframe_pack_ref as R
import test_abi

EXT_HEADER = "ext/hsr_keyframe_pack.h"
NAMES = ["hsr_keyframe_pack_scratch_bytes", "hsr_keyframe_pack", "hsr_keyframe_unpack"]
FP, VP = ("pointer", "float"), ("pointer", "void")
U8, U16, I64 = ("pointer", "uint8_t"), ("pointer", "uint16_t"), ("pointer", "int64_t")


def test_keyframe_pack_abi_exported_and_bound():
    from diff_gaussian_rasterization import _abi
    protos = test_abi._prototypes([EXT_HEADER])
    assert [s[0] for s in _abi.HEADERS[EXT_HEADER]] == list(protos) == NAMES
    assert all(n.startswith("hsr_keyframe_") for n in NAMES)
    assert protos["hsr_keyframe_pack_scratch_bytes"][1:] == ("size_t", ["int", "int", "int"])
    assert protos["hsr_keyframe_pack"][1:] == ("int", ["int", "int", FP, FP, "int", I64, "double", U8, U16, U16, ("pointer", "uint32_t"),
                                                       ("pointer", "char"), "size_t", VP])
    assert protos["hsr_keyframe_unpack"][1:] == ("int", ["int", "int", U8, U16, "int", U16, "double", FP, FP, I64, VP])
    from hsr_utils import checkpoint
    src = test_abi._source(EXT_HEADER)
    assert "#define HSR_KEYFRAME_MAX_SIDE 16384" in src and checkpoint.MAX_SIDE == 16384
    assert "#define HSR_KEYFRAME_MAX_PLANES 17" in src and checkpoint.MAX_PLANES == 17


def test_names_are_reached_lazily_from_the_package():
    import hsr_utils
    from hsr_utils import checkpoint
    assert set(hsr_utils._CHECKPOINT) <= set(checkpoint.__all__)
    for name in hsr_utils._CHECKPOINT:
        assert getattr(hsr_utils, name) is getattr(checkpoint, name), name
    assert callable(hsr_utils.SlamSession.save_checkpoint) and callable(hsr_utils.SlamSession.load_checkpoint)


# ---- refusals: dummy non-device pointers that are never followed -------------------------------------------------------------------------
def pack_call(lib, H=5, W=7, color=4096, depth=8192, L=2, labels=12288, depth_scale=6553.5, out_color=16384, out_depth=20480,
              out_labels=24576, lossy=28672, scratch=1 << 20, scratch_bytes=1 << 16):
    return lib.hsr_keyframe_pack(H, W, color, depth, L, labels, depth_scale, out_color, out_depth, out_labels, lossy, scratch, scratch_bytes, None)


def unpack_call(lib, H=5, W=7, color=4096, depth=8192, L=2, labels=12288, depth_scale=6553.5, out_color=16384, out_depth=20480,
                out_labels=24576):
    return lib.hsr_keyframe_unpack(H, W, color, depth, L, labels, depth_scale, out_color, out_depth, out_labels, None)


SHARED_REFUSALS = (
    [(dict(H=0), b"sides must be 1..16384; got 0x7"), (dict(W=0), b"got 5x0"), (dict(H=-3), b"sides must be"), (dict(H=16385), b"sides must be"),
     (dict(W=16385), b"sides must be"), (dict(L=-1), b"L must be 0..17; got -1"), (dict(L=18), b"L must be 0..17; got 18")]
    + [(dict(depth_scale=s), b"depth_scale must be finite and non-zero") for s in (0.0, -0.0, float("inf"), float("-inf"), float("nan"))]
    + [(dict(out_color=None), b"colour or depth given without its output"), (dict(out_depth=None), b"colour or depth given without its output"),
       (dict(labels=None), b"labels given without an output (or the reverse)"), (dict(out_labels=None), b"labels given without an output"),
       (dict(L=0), b"L=0 takes both NULL"), (dict(L=0, labels=None), b"L=0 takes both NULL"), (dict(L=0, out_labels=None), b"L=0 takes both NULL"),
       (dict(L=2, labels=None, out_labels=None), b"L=2 takes both pointers"),
       (dict(color=None, depth=None, L=0, labels=None, out_labels=None), b"nothing to do")]
)
PACK_REFUSALS = SHARED_REFUSALS + [
    (dict(lossy=None), b"NULL lossy"), (dict(scratch=None), b"scratch too small"),
    (dict(scratch_bytes=255), b"scratch too small: 256 bytes needed, 255 given"), (dict(scratch_bytes=0), b"scratch too small"),
    (dict(scratch=(1 << 20) + 2), b"not 4-byte aligned"),
    (dict(H=680, W=1200, L=5, scratch_bytes=28671), b"scratch too small: 28928 bytes needed, 28671 given"),
]


@pytest.mark.parametrize("overrides,message", PACK_REFUSALS, ids=["%d" % i for i in range(len(PACK_REFUSALS))])
def test_keyframe_pack_refuses_before_any_device_work(overrides, message):
    from diff_gaussian_rasterization import _abi
    rc = pack_call(_abi.lib, **overrides)
    err = _abi.lib.hsr_last_error()
    assert rc == -1 and err.startswith(b"keyframe_pack: ") and message in err, (overrides, rc, err)


@pytest.mark.parametrize("overrides,message", SHARED_REFUSALS, ids=["%d" % i for i in range(len(SHARED_REFUSALS))])
def test_keyframe_unpack_refuses_before_any_device_work(overrides, message):
    from diff_gaussian_rasterization import _abi
    rc = unpack_call(_abi.lib, **overrides)
    err = _abi.lib.hsr_last_error()
    assert rc == -1 and err.startswith(b"keyframe_unpack: ") and message in err, (overrides, rc, err)


def test_scratch_sizes():
    from diff_gaussian_rasterization import _abi
    need = _abi.lib.hsr_keyframe_pack_scratch_bytes
    # one 32-bit count per workgroup of 1024 values and plane, 4 + L planes, rounded up to 256 bytes
    assert [need(1, 1, 0), need(32, 32, 0), need(25, 41, 0), need(25, 41, 17), need(96, 128, 5)] == [256, 256, 256, 256, 512]
    assert need(680, 1200, 5) == 28928 and need(680, 1200, 0) == 12800      # ceil(816000 / 1024) = 797 workgroups per plane
    assert need(16384, 16384, 17) == 21 * (1 << 18) * 4
    assert need(0, 5, 0) > 0 and need(5, 5, 18) > 0 and need(5, 16385, 0) > 0


# ---- the condition that makes the exactness claim testable ---------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [6553.5, 1000.0, 5000.0])
def test_every_sensor_code_round_trips_through_the_restatement(scale):
    grey = R.ingest_colour(np.arange(256, dtype=np.float32))
    codes, lossy = R.pack_colour(grey)
    assert lossy == 0 and np.array_equal(codes, np.arange(256, dtype=np.uint8))
    assert np.array_equal(R.ingest_colour(codes.astype(np.float32)).view(np.uint32), grey.view(np.uint32))
    depth = R.ingest_depth(np.arange(65536, dtype=np.float64), scale)
    q, lossy = R.pack_depth(depth, scale)
    assert lossy == 0 and np.array_equal(q, np.arange(65536, dtype=np.uint16))
    assert np.array_equal(R.ingest_depth(q.astype(np.float64), scale).view(np.uint32), depth.view(np.uint32))
    labels, lossy = R.pack_labels(np.array([0, 1, 65535], np.int64))
    assert lossy == 0 and labels.tolist() == [0, 1, 65535]


def test_the_restatement_counts_what_does_not_round_trip():
    nan, inf = np.float32("nan"), np.float32("inf")
    c = np.array([0.0, 1.0, 0.5, nan, inf, -inf, -0.0, 1.0000001, -1e-9, np.float32(128) / np.float32(255)], np.float32)
    codes, lossy = R.pack_colour(c)
    assert codes.tolist() == [0, 255, 128, 0, 255, 0, 0, 255, 0, 128] and lossy == 7
    scale = 6553.5
    d = np.array([0.0, R.ingest_depth(1234, scale), (R.ingest_depth(7, scale) + R.ingest_depth(8, scale)) / 2, 65536 / scale, nan, inf, -0.0,
                  -1.0], np.float32)
    q, lossy = R.pack_depth(d, scale)
    assert q[:2].tolist() == [0, 1234] and q[2] in (7, 8) and q[3:].tolist() == [65535, 0, 65535, 0, 0] and lossy == 6
    labels, lossy = R.pack_labels(np.array([-1, 65535, 65536, 2 ** 40, -2 ** 40], np.int64))
    assert labels.tolist() == [0, 65535, 65535, 65535, 0] and lossy == 4


# ---- config ------------------------------------------------------------------------------------------------------------------------------------
def _config(**over):
    lrs_t = dict(means3D=0.0, rgb_colors=0.0, unnorm_rotations=0.0, logit_opacities=0.0, log_scales=0.0, cam_unnorm_rots=4e-4, cam_trans=2e-3)
    lrs_m = dict(means3D=1e-4, rgb_colors=2.5e-3, unnorm_rotations=1e-3, logit_opacities=0.05, log_scales=1e-3, cam_unnorm_rots=0.0, cam_trans=0.0)
    cfg = dict(map_every=1, keyframe_every=3, mapping_window_size=4, data=dict(num_frames=8),
               tracking=dict(num_iters=5, lrs=lrs_t, loss_weights=dict(im=0.5, depth=1.0), sil_thres=0.99),
               mapping=dict(num_iters=5, lrs=lrs_m, loss_weights=dict(im=0.5, depth=1.0), sil_thres=0.5))
    cfg.update(over)
    return cfg


def test_checkpoint_config_keys():
    from hsr_utils import slam
    out = slam.normalize_config(_config())
    assert out["save_checkpoints"] is False and "checkpoint_interval" not in out and "workdir" not in out and "run_name" not in out
    full = dict(save_checkpoints=True, checkpoint_interval=100, workdir="w", run_name="r")
    out = slam.normalize_config(_config(**full))
    assert out["save_checkpoints"] is True and (out["checkpoint_interval"], out["workdir"], out["run_name"]) == (100, "w", "r")
    for key in ("checkpoint_interval", "workdir", "run_name"):
        with pytest.raises(KeyError, match=key):
            slam.normalize_config(_config(**{k: v for k, v in full.items() if k != key}))
        slam.normalize_config(_config(**{k: v for k, v in full.items() if k not in (key, "save_checkpoints")}))      # not read unless saving
    with pytest.raises(ValueError, match="keyframe_store"):
        slam.SlamSession(_config(), torch.eye(3), torch.eye(4), cam=None, keyframe_store="zip")
    assert slam.SlamSession(_config(), torch.eye(3), torch.eye(4), cam=None).keyframe_store == "raw"


# ---- save and load on a hand-built host session ----------------------------------------------------------------------------------------
H, W, P, FRAMES_DONE = 4, 6, 9, 5


def _host_session(semantic, seed=0):
    """a session as it stands after FRAMES_DONE frames, built by hand on the host: no kernel has run"""
    from hsr_utils import slam
    g = torch.Generator().manual_seed(seed)
    cam = types.SimpleNamespace(image_height=H, image_width=W, viewmatrix=torch.eye(4)[None])
    over = dict(num_semantic=[2, 3], model=dict(flag_use_embedding=1), num_semantic_class=4) if semantic else {}
    s = slam.SlamSession(_config(**over), torch.eye(3), torch.eye(4), cam)
    rows = {"means3D": 3, "rgb_colors": 3, "unnorm_rotations": 4, "logit_opacities": 1, "log_scales": 1}
    if semantic:
        rows["semantic"] = 5
    s.params = {k: torch.nn.Parameter(torch.randn(P, n, generator=g)) for k, n in rows.items()}
    s.params["cam_unnorm_rots"] = torch.nn.Parameter(torch.randn(1, 4, 8, generator=g))
    s.params["cam_trans"] = torch.nn.Parameter(torch.randn(1, 3, 8, generator=g))
    s.variables = {k: torch.rand(P, generator=g) for k in ("max_2D_radius", "means2D_gradient_accum", "denom")}
    s.variables["timestep"] = torch.randint(0, FRAMES_DONE, (P,), generator=g).float()
    s.variables["scene_radius"] = torch.tensor(1.75)
    s.variables["means2D"], s.variables["seen"] = torch.zeros(P, 3), torch.ones(P, dtype=torch.bool)      # per-iteration: not saved
    s.gt_w2c_all_frames = [torch.randn(4, 4, generator=g) if t != 2 else None for t in range(FRAMES_DONE)]
    for t in (0, 2):
        kf = {"id": t, "est_w2c": torch.randn(4, 4, generator=g), "color": torch.rand(3, H, W, generator=g),
              "depth": torch.rand(1, H, W, generator=g), "cam": cam, "intrinsics": s.intrinsics}
        if semantic:
            kf["label_gt"] = torch.randint(0, 3, (3, H, W), generator=g) if t == 0 else None
        s.keyframe_list.append(kf)
        s.keyframe_time_indices.append(t)
    if semantic:
        s.mlp = torch.nn.Conv2d(5, 4, kernel_size=1)
        s.mlp_optimizer = torch.optim.Adam(s.mlp.parameters(), lr=5e-4)
        s.mlp(torch.randn(1, 5, H, W, generator=g)).square().sum().backward()
        s.mlp_optimizer.step()
        s.mlp_optimizer.zero_grad()
    return s


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = a.detach(), b.detach()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))      # bit patterns


@pytest.mark.parametrize("semantic", [False, True], ids=["plain", "semantic"])
def test_host_session_round_trips_bit_for_bit(tmp_path, semantic, monkeypatch):
    import time
    from hsr_utils import map_io, slam
    a = _host_session(semantic)
    np.random.seed(11)
    torch.manual_seed(12)
    np.random.standard_normal()      # leaves a cached gaussian in the state
    np_before, torch_before = np.random.get_state(), torch.get_rng_state()
    kept = {k: v.detach().clone() for k, v in a.params.items()}
    monkeypatch.setattr(time, "time", lambda: 1.7e9)      # a zip member carries its time: both files of the comparison below get the same
    paths = a.save_checkpoint(str(tmp_path / "run"))
    assert [os.path.basename(p) for p in paths] == ["params4.npz", "keyframe_time_indices4.npy", "session4.npz"]
    map_io.save_params_ckpt(a.params, str(tmp_path / "ref"), 4)
    monkeypatch.undo()
    assert open(paths[0], "rb").read() == open(str(tmp_path / "ref" / "params4.npz"), "rb").read()
    assert np.load(paths[1]).tolist() == [0, 2]
    # saving drew from no stream and changed nothing
    assert all(np.array_equal(x, y) for x, y in zip(np_before, np.random.get_state())) and torch.equal(torch_before, torch.get_rng_state())
    assert all(torch.equal(a.params[k].detach(), kept[k]) for k in kept) and "color" in a.keyframe_list[0]
    z = np.load(paths[2], allow_pickle=False)      # arrays only
    assert "var.means2D" not in z.files and "var.seen" not in z.files and "kf0.color_raw" in z.files and "kf0.color_u8" not in z.files
    next_np, next_torch = np.random.randint(0, 1 << 30, 4), torch.randint(0, 1 << 30, (4,))

    np.random.seed(99)
    torch.manual_seed(98)
    over = dict(num_semantic=[2, 3], model=dict(flag_use_embedding=1), num_semantic_class=4) if semantic else {}
    b = slam.SlamSession(_config(**over), torch.eye(3), torch.eye(4), a.cam)
    assert b.load_checkpoint(str(tmp_path / "run"), 4) == 5
    assert np.array_equal(np.random.randint(0, 1 << 30, 4), next_np) and torch.equal(torch.randint(0, 1 << 30, (4,)), next_torch)
    assert set(b.params) == set(a.params)
    for k in a.params:
        assert isinstance(b.params[k], torch.nn.Parameter) and b.params[k].requires_grad and _same(a.params[k], b.params[k]), k
    assert set(b.variables) == set(a.variables) - {"means2D", "seen"}
    for k in b.variables:
        assert _same(a.variables[k], b.variables[k]), k
    assert len(b.gt_w2c_all_frames) == FRAMES_DONE and b.gt_w2c_all_frames[2] is None
    assert all(_same(x, y) for x, y in zip(a.gt_w2c_all_frames, b.gt_w2c_all_frames))
    assert b.keyframe_time_indices == [0, 2] and [kf["id"] for kf in b.keyframe_list] == [0, 2]
    for ka, kb in zip(a.keyframe_list, b.keyframe_list):
        assert _same(ka["est_w2c"], kb["est_w2c"]) and _same(ka["color"], kb["color"]) and _same(ka["depth"], kb["depth"])
        assert kb["cam"] is b.cam and kb["intrinsics"] is b.intrinsics
        if semantic:
            assert "label_gt" in kb and _same(ka["label_gt"], kb["label_gt"])
        else:
            assert "label_gt" not in kb
    if semantic:
        for (n, pa), (_n, pb) in zip(a.mlp.named_parameters(), b.mlp.named_parameters()):
            assert _same(pa, pb), n
            sa, sb = a.mlp_optimizer.state[pa], b.mlp_optimizer.state[pb]
            assert set(sa) == set(sb) == {"step", "exp_avg", "exp_avg_sq"} and all(_same(sa[m], sb[m]) for m in sa), n
    else:
        assert b.mlp is None and b.mlp_optimizer is None
    # the next step() takes frame 5
    with pytest.raises(RuntimeError, match="frame 4 stepped after 5 frames"):
        b.step({"id": 4})


def test_load_refuses_a_mismatch_and_a_used_session(tmp_path):
    from hsr_utils import slam
    a = _host_session(False)
    a.save_checkpoint(str(tmp_path))
    with pytest.raises(ValueError, match="stands after frame 4"):
        a.save_checkpoint(str(tmp_path), 3)
    with pytest.raises(RuntimeError, match="freshly constructed"):
        a.load_checkpoint(str(tmp_path), 4)
    cases = ((dict(data=dict(num_frames=9)), a.cam, "num_frames = 8, this session has 9"),
             (dict(num_semantic=5), a.cam, "num_semantic = -1, this session has 5"),
             (dict(gaussian_distribution="anisotropic"), a.cam, "scale_columns = 1, this session has 3"),
             ({}, types.SimpleNamespace(image_height=H + 1, image_width=W, viewmatrix=torch.eye(4)), "height = 4, this session has 5"),
             ({}, types.SimpleNamespace(image_height=H, image_width=W + 2, viewmatrix=torch.eye(4)), "width = 6, this session has 8"))
    for over, cam, message in cases:
        b = slam.SlamSession(_config(**over), torch.eye(3), torch.eye(4), cam)
        with pytest.raises(RuntimeError, match=message):
            b.load_checkpoint(str(tmp_path), 4)
        assert b.params is None and b.keyframe_list == []
    os.rename(str(tmp_path / "session4.npz"), str(tmp_path / "session3.npz"))
    os.rename(str(tmp_path / "params4.npz"), str(tmp_path / "params3.npz"))
    b = slam.SlamSession(_config(), torch.eye(3), torch.eye(4), a.cam)
    with pytest.raises(RuntimeError, match="frames = 5, this session has 4"):      # the frame count is part of the fingerprint
        b.load_checkpoint(str(tmp_path), 3)
    with pytest.raises(FileNotFoundError):
        b.load_checkpoint(str(tmp_path), 7)
    os.remove(str(tmp_path / "session3.npz"))
    with pytest.raises(RuntimeError, match="needs frames="):                        # the reference's kind of checkpoint
        b.load_checkpoint(str(tmp_path), 3)
    fresh = slam.SlamSession(_config(), torch.eye(3), torch.eye(4), a.cam)
    with pytest.raises(RuntimeError, match="before the first frame"):
        fresh.save_checkpoint(str(tmp_path))


def test_pack_keyframe_has_no_cpu_path():
    from hsr_utils import checkpoint
    with pytest.raises(RuntimeError, match="no CPU path"):
        checkpoint.pack_keyframe(torch.zeros(3, H, W), torch.zeros(1, H, W))
    with pytest.raises(RuntimeError, match=r"color must be \[3,H,W\]"):
        checkpoint.pack_keyframe(torch.zeros(3, H, W + 1), torch.zeros(1, H, W))
    with pytest.raises(RuntimeError, match=r"labels must be \[L,4,6\]"):
        checkpoint.pack_keyframe(torch.zeros(3, H, W), torch.zeros(1, H, W), torch.zeros(H, W, dtype=torch.int64))
    pk = checkpoint.raw_keyframe(torch.rand(3, H, W), torch.rand(1, H, W))
    assert pk.exact == {"color": False, "depth": False} and pk.lossy_counts is None
    color, depth, labels = checkpoint.unpack_keyframe(pk)
    assert color is pk.raw["color"] and depth is pk.raw["depth"] and labels is None
