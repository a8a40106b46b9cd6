"""GPU suite for a session's checkpoint and resume (hsr_utils.checkpoint, SlamSession.save_checkpoint / load_checkpoint) and the packed
keyframe store (SlamSession(..., keyframe_store="packed")).

The sequence is built as tests/test_gpu_slam_session.py builds its own, smaller: 6 frames at 64x48 rendered from a hidden map along a smooth
path, keyframe_every = 2, map_every = 1, 6 tracking and 16 mapping iterations (the leaf head joins the loss from iteration 14 on, so its
Adam state exists).  Two cases: a 2-level tree (2 + 2 classes) with the leaf head, and no semantics.  The colour planes are quantised to
grey levels over 255 and the depth to codes over png_depth_scale = 6553.5, as ingest() at sensor size leaves them, so that the packed
store really packs.

What is compared bit for bit is what is deterministic: the restored state, a forward render, and after a further step the integers
(the window, the Gaussian count, the iteration count, the keyframe ids).  The optimised floats of a further step are NOT compared: the
backward's float atomics make two runs differ."""
import os
import random

import numpy as np
import pytest
import torch

import keyframe_pack_ref as R

pytestmark = pytest.mark.gpu

W, H, LEVELS, FRAMES, SCALE = 64, 48, [2, 2], 6, 6553.5
K = sum(LEVELS)


def _hidden_map(kmat):
    from hsr_utils import make_scene
    P = 14000
    sc = make_scene(P, W, H, K, kmat, seed=7, kind="slam")
    fx, fy, cx, cy = kmat[0][0], kmat[1][1], kmat[0][2], kmat[1][2]
    g = torch.Generator().manual_seed(8)
    u = torch.rand(P, generator=g) * (W + 40) - 20
    v = torch.rand(P, generator=g) * (H + 40) - 20
    z = 2.5 + 0.35 * torch.sin(u / 9.0) + 0.25 * torch.cos(v / 7.0)
    means = torch.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], dim=1).float()
    colour = 0.5 + 0.25 * torch.stack([torch.sin(u / 5.0), torch.cos(v / 4.0), torch.sin((u + v) / 6.0)], dim=1) + 0.25 * (sc["colors_precomp"] - 0.5)
    sem = sc["semantics_precomp"].clone()
    sem[:, 0] += (u > W / 2).float()
    sem[:, 2] += (v > H / 2).float()
    scale = (1.3 * z / (0.5 * (fx + fy))).float()
    return {"means3D": means, "rgb_colors": colour.float().clamp(0, 1), "unnorm_rotations": sc["rotations"],
            "logit_opacities": torch.full((P, 1), 3.0), "log_scales": scale.log()[:, None], "semantic": sem}


@pytest.fixture(scope="module")
def sequence():
    """(cam, intrinsics, frames): every frame with 'semantic_label_gt' [3,H,W] (two tree levels and the leaf plane); computed once"""
    from diff_gaussian_rasterization import GaussianRasterizer_semantic
    from hsr_utils import setup_camera, slam, slam_helpers as SH
    from hsr_utils.camera import replica_intrinsics
    kmat = replica_intrinsics(W, H)
    cam = setup_camera(W, H, kmat, np.eye(4), device="cuda")
    hidden = {k: v.cuda().contiguous() for k, v in _hidden_map(kmat).items()}
    rots, trans = torch.zeros(1, 4, FRAMES), torch.zeros(1, 3, FRAMES)
    for t in range(FRAMES):
        q = torch.tensor([1.0, 0.0015 * t, -0.0030 * t, 0.0010 * t])
        rots[0, :, t] = q / q.norm()
        trans[0, :, t] = torch.tensor([0.018 * t, -0.008 * t, 0.012 * t])
    hidden["cam_unnorm_rots"], hidden["cam_trans"] = rots.cuda(), trans.cuda()
    frames = []
    with torch.no_grad():
        for t in range(FRAMES):
            rv = SH.transformed_params2rendervar_semantic(hidden, SH.transform_to_frame(hidden, t, False, False))
            im, _radius, sem, depth, _median, _opac = GaussianRasterizer_semantic(raster_settings=cam)(**rv)
            l0, l1 = sem[:2].argmax(dim=0), sem[2:4].argmax(dim=0)
            # what a sensor would have delivered: 8-bit grey levels and 16-bit depth codes through the ingest expressions
            grey = torch.round(im.clamp(0, 1) * 255).cpu().numpy().astype(np.float32)
            code = torch.round(depth.double() * SCALE).clamp(0, 65535).cpu().numpy()
            frames.append({"id": t, "im": torch.from_numpy(R.ingest_colour(grey)).cuda(), "depth": torch.from_numpy(R.ingest_depth(code, SCALE)).cuda(),
                           "semantic_label_gt": torch.stack([l0, l1, 2 * l0 + l1]), "gt_w2c": slam.frame_w2c(hidden, t)})
    return cam, torch.tensor(kmat, dtype=torch.float32, device="cuda"), frames


def _config(semantic, **over):
    zero = dict(means3D=0.0, rgb_colors=0.0, unnorm_rotations=0.0, logit_opacities=0.0, log_scales=0.0, semantic=0.0)
    cfg = dict(
        num_frames=FRAMES, map_every=1, keyframe_every=2, mapping_window_size=4, scene_radius_depth_ratio=3, png_depth_scale=SCALE,
        mean_sq_dist_method="projective", gaussian_distribution="isotropic",
        tracking=dict(num_iters=6, use_gt_poses=False, forward_prop=True, use_sil_for_loss=True, sil_thres=0.9, use_l1=True,
                      ignore_outlier_depth_loss=False, loss_weights=dict(im=0.5, depth=1.0), lrs=dict(zero, cam_unnorm_rots=4e-4, cam_trans=2e-3)),
        mapping=dict(num_iters=16, add_new_gaussians=True, sil_thres=0.5, use_l1=True, use_sil_for_loss=False, ignore_outlier_depth_loss=False,
                     loss_weights=dict(im=0.5, depth=1.0, sem=0.05),
                     lrs=dict(means3D=1e-4, rgb_colors=2.5e-3, unnorm_rotations=1e-3, logit_opacities=0.05, log_scales=1e-3, semantic=2.5e-3,
                              cam_unnorm_rots=0.0, cam_trans=0.0),
                     prune_gaussians=False, use_gaussian_splatting_densification=False))
    if semantic:
        cfg.update(num_semantic=LEVELS, num_semantic_class=4, model=dict(flag_use_embedding=1))
    cfg.update(over)
    return cfg


def _session(sequence, semantic, store="raw", **over):
    from hsr_utils import SlamSession
    cam, intrinsics, _frames = sequence
    return SlamSession(_config(semantic, **over), intrinsics, torch.eye(4, device="cuda"), cam, keyframe_store=store)


def _frames_of(sequence, semantic):
    frames = sequence[2]
    return frames if semantic else [{k: v for k, v in f.items() if k != "semantic_label_gt"} for f in frames]


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = a.detach(), b.detach()
    if a.dtype != b.dtype or a.shape != b.shape or a.device != b.device:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))      # bit patterns


def _planes(kf):
    from hsr_utils import checkpoint
    return checkpoint.keyframe_planes(kf)


def _rng_state():
    return np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state()


def _set_rng_state(state):
    np.random.set_state(state[0])
    torch.set_rng_state(state[1])
    torch.cuda.set_rng_state(state[2])


def _deterministic(s):
    return (s.last_window, int(s.params["means3D"].shape[0]), s.num_tracking_iters, list(s.keyframe_time_indices))


@pytest.fixture(scope="module", params=[True, False], ids=["tree+leaf", "plain"])
def saved(request, sequence, tmp_path_factory):
    """session A stepped through frames 0..3 and saved: (semantic, A, directory, the random streams as they stood at the save)"""
    semantic = request.param
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    a = _session(sequence, semantic)
    for frame in _frames_of(sequence, semantic)[:4]:
        a.step(frame)
    directory = str(tmp_path_factory.mktemp("ckpt"))
    state = _rng_state()
    paths = a.save_checkpoint(directory)
    assert [os.path.basename(p) for p in paths] == ["params3.npz", "keyframe_time_indices3.npy", "session3.npz"]
    assert all(np.array_equal(x, y) for x, y in zip(state[0], np.random.get_state()))      # saving drew from no stream
    assert torch.equal(state[1], torch.get_rng_state()) and torch.equal(state[2], torch.cuda.get_rng_state())
    return semantic, a, directory, state


def test_load_restores_the_session_bit_for_bit(sequence, saved):
    semantic, a, directory, _state = saved
    b = _session(sequence, semantic)
    assert b.load_checkpoint(directory, 3) == 4
    assert set(a.params) == set(b.params) and all(_same(a.params[k], b.params[k]) and b.params[k].requires_grad for k in a.params)
    assert set(b.variables) == set(a.variables) - {"means2D", "seen"} and all(_same(a.variables[k], b.variables[k]) for k in b.variables)
    assert a.keyframe_time_indices == b.keyframe_time_indices == [0, 1, 3]
    assert len(b.gt_w2c_all_frames) == 4 and all(_same(x, y) for x, y in zip(a.gt_w2c_all_frames, b.gt_w2c_all_frames))
    assert len(a.keyframe_list) == len(b.keyframe_list) == 3
    for ka, kb in zip(a.keyframe_list, b.keyframe_list):
        assert ka["id"] == kb["id"] and _same(ka["est_w2c"], kb["est_w2c"]) and kb["cam"] is b.cam
        assert _same(ka["color"], kb["color"]) and _same(ka["depth"], kb["depth"]) and _same(ka.get("label_gt"), kb.get("label_gt"))
        assert ("label_gt" in kb) == semantic
    z = np.load(os.path.join(directory, "session3.npz"), allow_pickle=False)
    for i in range(3):      # the sequence is sensor-exact: every group went to disk as codes
        assert {"kf%d.color_u8" % i, "kf%d.depth_u16" % i} <= set(z.files) and ("kf%d.labels_u16" % i in z.files) == semantic
        assert not [k for k in z.files if k.startswith("kf%d." % i) and k.endswith("_raw")]
    if semantic:
        assert a.mlp is not b.mlp
        for (n, pa), (_n, pb) in zip(a.mlp.named_parameters(), b.mlp.named_parameters()):
            sa, sb = a.mlp_optimizer.state[pa], b.mlp_optimizer.state[pb]
            assert _same(pa, pb) and set(sa) == set(sb) == {"step", "exp_avg", "exp_avg_sq"} and all(_same(sa[m], sb[m]) for m in sa), n
    else:
        assert b.mlp is None
    ra, rb = a.render(3), b.render(3)      # the forward is deterministic
    assert all(_same(x, y) for x, y in zip(ra, rb))


def test_a_resumed_session_takes_the_next_frame_as_the_saved_one_does(sequence, saved):
    semantic, a, directory, state = saved
    frame = _frames_of(sequence, semantic)[4]
    b = _session(sequence, semantic)
    np.random.seed(77); torch.manual_seed(78)      # the load must bring the saved streams back
    b.load_checkpoint(directory, 3)
    assert all(np.array_equal(x, y) for x, y in zip(state[0], np.random.get_state()))
    assert torch.equal(state[1], torch.get_rng_state()) and torch.equal(state[2], torch.cuda.get_rng_state())
    b.step(frame)
    _set_rng_state(state)
    a.step(frame)      # `saved` is used up by this test: the ones below load from its files only
    assert _deterministic(a) == _deterministic(b)
    assert a.last_window[0][-1] == 4 and a.keyframe_time_indices == [0, 1, 3, 4] and a.num_tracking_iters == 6


@pytest.mark.parametrize("semantic", [True, False], ids=["tree+leaf", "plain"])
def test_packed_store_runs_the_same_sequence(sequence, semantic, tmp_path):
    frames = _frames_of(sequence, semantic)
    runs = {}
    for store in ("raw", "packed"):
        torch.manual_seed(0); np.random.seed(0); random.seed(0)
        s = _session(sequence, semantic, store)
        log = []
        for frame in frames[:5]:
            s.step(frame)
            log.append(_deterministic(s))
        runs[store] = (s, log)
    (raw, raw_log), (packed, packed_log) = runs["raw"], runs["packed"]
    assert raw_log == packed_log
    assert [kf["id"] for kf in packed.keyframe_list] == [0, 1, 3, 4]
    for kr, kp in zip(raw.keyframe_list, packed.keyframe_list):
        assert "color" not in kp and "depth" not in kp and "label_gt" not in kp and kr["id"] == kp["id"]
        assert kp["packed"].exact == ({"color": True, "depth": True, "labels": True} if semantic else {"color": True, "depth": True})
        color, depth, labels = _planes(kp)
        assert _same(color, kr["color"]) and _same(depth, kr["depth"]) and _same(labels, kr.get("label_gt"))
    per_pixel = 3 + 2 + (2 * 3 if semantic else 0)
    assert sum(kf["packed"].nbytes() for kf in packed.keyframe_list) == 4 * H * W * per_pixel
    # a packed session saves and loads as packed, and into a raw session as raw
    packed.save_checkpoint(str(tmp_path))
    for store in ("packed", "raw"):
        b = _session(sequence, semantic, store)
        assert b.load_checkpoint(str(tmp_path), 4) == 5
        for kr, kb in zip(raw.keyframe_list, b.keyframe_list):
            assert ("packed" in kb) == (store == "packed")
            assert all(_same(x, y) for x, y in zip(_planes(kb), (kr["color"], kr["depth"], kr.get("label_gt"))))


def test_a_checkpoint_of_the_references_kind_loads_from_frames(sequence, saved, tmp_path):
    semantic, _a, directory, _state = saved
    import shutil
    for name in ("params3.npz", "keyframe_time_indices3.npy"):      # no session3.npz: what the reference writes
        shutil.copy(os.path.join(directory, name), str(tmp_path / name))
    frames = _frames_of(sequence, semantic)
    asked = []

    def supply(i):
        asked.append(i)
        return frames[i]
    b = _session(sequence, semantic)
    assert b.load_checkpoint(str(tmp_path), 3, frames=supply) == 3
    assert asked == [0, 0, 1, 2]      # frame 0 for the initialisation, then every frame before the checkpoint
    saved_params = np.load(str(tmp_path / "params3.npz"))
    assert set(saved_params.files) == set(b.params)
    assert all(np.array_equal(saved_params[k], b.params[k].detach().cpu().numpy()) and b.params[k].requires_grad for k in b.params)
    P = b.params["means3D"].shape[0]
    for k in ("max_2D_radius", "means2D_gradient_accum", "denom", "timestep"):
        assert b.variables[k].shape == (P,) and not bool(b.variables[k].any())
    assert float(b.variables["scene_radius"]) > 0
    assert b.keyframe_time_indices == [0, 1] and [kf["id"] for kf in b.keyframe_list] == [0, 1]      # the list is cut to entries < 3
    for kf in b.keyframe_list:
        f = frames[kf["id"]]
        assert kf["color"] is f["im"] and kf["depth"] is f["depth"] and _same(kf["est_w2c"], b.estimated_w2c()[kf["id"]])
        assert ("label_gt" in kf) == semantic and (not semantic or kf["label_gt"] is f["semantic_label_gt"])
    assert len(b.gt_w2c_all_frames) == 3 and all(x is frames[i]["gt_w2c"] for i, x in enumerate(b.gt_w2c_all_frames))
    with pytest.raises(RuntimeError, match="frame 4 stepped after 3 frames"):
        b.step(frames[4])
    b.step(frames[3])      # the next accepted frame is 3
    assert b.keyframe_time_indices == [0, 1, 3] and b.last_window[0][-1] == 3


def test_step_saves_at_the_multiples_of_the_interval(sequence, tmp_path):
    frames = _frames_of(sequence, False)
    torch.manual_seed(0); np.random.seed(0)
    over = dict(save_checkpoints=True, checkpoint_interval=2, workdir=str(tmp_path), run_name="run")
    over["tracking"] = dict(_config(False)["tracking"], num_iters=2)
    over["mapping"] = dict(_config(False)["mapping"], num_iters=2)
    s = _session(sequence, False, **over)
    seen = []
    for frame in frames[:5]:
        s.step(frame)
        seen.append(sorted(os.listdir(str(tmp_path / "run"))) if os.path.isdir(str(tmp_path / "run")) else [])
    files = lambda ts: sorted(n % t for t in ts for n in ("keyframe_time_indices%d.npy", "params%d.npz", "session%d.npz"))      # noqa: E731
    assert seen == [files([0]), files([0]), files([0, 2]), files([0, 2]), files([0, 2, 4])]
    b = _session(sequence, False)
    assert b.load_checkpoint(str(tmp_path / "run"), 2) == 3 and len(b.keyframe_list) == 2
