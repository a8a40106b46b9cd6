"""GPU suite for SlamSession with tracking and densification resolutions of their own (scripts/hierslam.py:1543-1563, :1680-1699,
:1792-1799, :1933-1941, :435-456).

The sequence is the recipe of tests/test_gpu_slam_session.py at twice the size: 6 frames at 192x128, K = 4 in a 2 + 2 tree, the same
camera path, seeds and config, the hidden map's P scaled with the pixel count (x 4) so that it still covers every pixel.  Tracking and
densification both run at 96x64, the size at which that suite shows this tracker converges.

Conditions (the figures are printed; the first MI355X run's are in profiles/multires_gpu.log):
   1. every tracking iteration's loss sees [3,64,96] images, every mapping iteration's [3,128,192] (the session's loss methods, wrapped);
   2. every keyframe's stored colour and depth are 128x192;
   3. exactly one resample launch per stepped frame (slam.resample_frame, wrapped);
   4. the ATE is finite and lower than that of the same session with 0 tracking iterations;
   5. after step(frame 0) the map has as many Gaussians as the nearest-resampled 64x96 depth has positive pixels (6144 with full
      coverage; 24576 without the keys);
   6. the first-frame map is bit-equal to map_init_frame on resample_frame's output with densify_intrinsics: scene_radius after
      step(frame 0); means3D and log_scales as initialize() returns them inside step(frame 0) — that step goes on to map frame 0, and
      15 mapping iterations with non-zero learning rates move both, so the parameters after the whole step are no longer the map_init rows;
   7. the last frame's full-resolution PSNR is higher after its mapping step than before;
   8. the row counts of parameters, Adam moments and bookkeeping agree after every step;
   9. a session whose keys name the frame's own size has tracking_cam is cam and densify_cam is cam and launches no resample;
  10. caller-supplied tracking tensors are used in place of the resample (a constant colour, seen in the wrapped loss); a wrong shape raises."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

W, H, LEVELS, FRAMES = 192, 128, [2, 2], 6
TW, TH = 96, 64
K = sum(LEVELS)


def _intrinsics():
    from hsr_utils.camera import replica_intrinsics
    return replica_intrinsics(W, H)


def _gt_path():
    """tests/test_gpu_slam_session.py: a constant twist (the image motion in pixels doubles with the size)"""
    rots, trans = torch.zeros(1, 4, FRAMES), torch.zeros(1, 3, FRAMES)
    for t in range(FRAMES):
        q = torch.tensor([1.0, 0.0015 * t, -0.0030 * t, 0.0010 * t])
        rots[0, :, t] = q / q.norm()
        trans[0, :, t] = torch.tensor([0.018 * t, -0.008 * t, 0.012 * t])
    return rots, trans


def _hidden_map(kmat):
    """that suite's hidden map with every length in pixels doubled: the same surface, colours and labels at twice the resolution"""
    from hsr_utils import make_scene
    P = 4 * 30000
    sc = make_scene(P, W, H, K, kmat, seed=7, kind="slam")
    fx, fy, cx, cy = kmat[0][0], kmat[1][1], kmat[0][2], kmat[1][2]
    g = torch.Generator().manual_seed(8)
    u = torch.rand(P, generator=g) * (W + 96) - 48
    v = torch.rand(P, generator=g) * (H + 96) - 48
    z = 2.5 + 0.35 * torch.sin(u / 18.0) + 0.25 * torch.cos(v / 14.0)
    means = torch.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], dim=1).float()
    colour = 0.5 + 0.25 * torch.stack([torch.sin(u / 10.0), torch.cos(v / 8.0), torch.sin((u + v) / 12.0)], dim=1) + 0.25 * (sc["colors_precomp"] - 0.5)
    sem = sc["semantics_precomp"].clone()
    sem[:, 0] += (u > W / 2).float()
    sem[:, 2] += (v > H / 2).float()
    scale = (1.3 * z / (0.5 * (fx + fy))).float()
    return {"means3D": means, "rgb_colors": colour.float().clamp(0, 1), "unnorm_rotations": sc["rotations"],
            "logit_opacities": torch.full((P, 1), 3.0), "log_scales": scale.log()[:, None], "semantic": sem}


@pytest.fixture(scope="module")
def sequence():
    from diff_gaussian_rasterization import GaussianRasterizer_semantic
    from hsr_utils import setup_camera, slam, slam_helpers as SH
    kmat = _intrinsics()
    cam = setup_camera(W, H, kmat, np.eye(4), device="cuda")
    hidden = {k: v.cuda().contiguous() for k, v in _hidden_map(kmat).items()}
    rots, trans = _gt_path()
    hidden["cam_unnorm_rots"], hidden["cam_trans"] = rots.cuda(), trans.cuda()
    frames = []
    with torch.no_grad():
        for t in range(FRAMES):
            rv = SH.transformed_params2rendervar_semantic(hidden, SH.transform_to_frame(hidden, t, False, False))
            im, _radius, sem, depth, _median, opac = GaussianRasterizer_semantic(raster_settings=cam)(**rv)
            assert float(opac.min()) > 0.9                          # the hidden map covers every pixel of every frame
            labels = torch.stack([sem[:2].argmax(dim=0), sem[2:4].argmax(dim=0)])
            frames.append({"id": t, "im": im.clamp(0, 1).contiguous(), "depth": depth.contiguous(), "semantic_label_gt": labels,
                           "gt_w2c": slam.frame_w2c(hidden, t)})
    return cam, torch.tensor(kmat, dtype=torch.float32, device="cuda"), frames


def _config(tracking_iters, sizes=((TH, TW), (TH, TW))):
    zero = dict(means3D=0.0, rgb_colors=0.0, unnorm_rotations=0.0, logit_opacities=0.0, log_scales=0.0, semantic=0.0)
    data = dict(num_frames=FRAMES)
    if sizes is not None:
        (data["tracking_image_height"], data["tracking_image_width"]), (data["densification_image_height"], data["densification_image_width"]) = sizes
    return dict(
        data=data, num_semantic=LEVELS, map_every=1, keyframe_every=2, mapping_window_size=4, scene_radius_depth_ratio=3,
        mean_sq_dist_method="projective", gaussian_distribution="isotropic",
        tracking=dict(num_iters=tracking_iters, use_gt_poses=False, forward_prop=True, use_sil_for_loss=True, sil_thres=0.9, use_l1=True,
                      ignore_outlier_depth_loss=False, loss_weights=dict(im=0.5, depth=1.0),
                      lrs=dict(zero, cam_unnorm_rots=4e-4, cam_trans=2e-3)),
        mapping=dict(num_iters=15, add_new_gaussians=True, sil_thres=0.5, use_l1=True, use_sil_for_loss=False, ignore_outlier_depth_loss=False,
                     loss_weights=dict(im=0.5, depth=1.0, sem=0.05),
                     lrs=dict(means3D=1e-4, rgb_colors=2.5e-3, unnorm_rotations=1e-3, logit_opacities=0.05, log_scales=1e-3, semantic=2.5e-3,
                              cam_unnorm_rots=0.0, cam_trans=0.0),
                     prune_gaussians=True, use_gaussian_splatting_densification=False,
                     pruning_dict=dict(start_after=0, remove_big_after=0, stop_after=20, prune_every=20, removal_opacity_threshold=0.005,
                                       final_removal_opacity_threshold=0.005, reset_opacities=False, reset_opacities_every=500)))


def _row_counts(s):
    from hsr_utils import slam_external as SE
    rows = {k: int(p.shape[0]) for k, p in s.params.items() if k not in SE.CAMERA_KEYS}
    rows.update({"var/" + k: int(s.variables[k].shape[0]) for k in SE.VARIABLE_KEYS})
    for group in s.optimizer.param_groups:
        if group["name"] in SE.CAMERA_KEYS:
            continue
        p = group["params"][0]
        assert p is s.params[group["name"]]
        st = s.optimizer.state.get(p, {})
        for m in ("exp_avg", "exp_avg_sq"):
            if m in st:
                rows["%s/%s" % (m, group["name"])] = int(st[m].shape[0])
    return rows


class _ResampleCounter:
    """slam.resample_frame, wrapped: the sizes asked for, per call"""

    def __init__(self, monkeypatch):
        from hsr_utils import slam
        self.calls, real = [], slam.resample_frame

        def counted(color, depth, sizes):
            self.calls.append([tuple(hw) for hw in sizes])
            return real(color, depth, sizes)
        monkeypatch.setattr(slam, "resample_frame", counted)


def _run_session(sequence, tracking_iters, counter, frames=None, sizes=((TH, TW), (TH, TW)), n_frames=FRAMES):
    from hsr_utils import SlamSession, evaluate
    cam, intrinsics, seq_frames = sequence
    frames = seq_frames if frames is None else frames
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    s = SlamSession(_config(tracking_iters, sizes), intrinsics, torch.eye(4, device="cuda"), cam)
    log = dict(psnr_before=[], psnr_after=[], rows=[], counts=[], tracking_shapes=[], mapping_shapes=[], tracking_gt=[], launches=[],
               init=None)

    def psnr(frame):
        im, depth, _opac, _sem = s.render(frame["id"])
        return evaluate.frame_metrics(im, frame["im"], depth, frame["depth"])[0]

    init_of, map_of, tloss_of, mloss_of = s.initialize, s.map_frame, s._tracking_loss, s._mapping_loss

    def initialize(frame):
        out = init_of(frame)
        log["init"] = {k: s.params[k].detach().clone() for k in ("means3D", "log_scales")}
        return out

    def tracking_loss(data, im, depth, opac):
        log["tracking_shapes"].append((tuple(im.shape), tuple(data["im"].shape), tuple(depth.shape), tuple(data["depth"].shape)))
        log["tracking_gt"].append(data["im"])
        return tloss_of(data, im, depth, opac)

    def mapping_loss(data, im, sem, depth, it):
        log["mapping_shapes"].append((tuple(im.shape), tuple(data["im"].shape), tuple(depth.shape), tuple(data["depth"].shape)))
        return mloss_of(data, im, sem, depth, it)

    def map_frame(frame):
        before = psnr(frame)
        map_of(frame)
        log["psnr_before"].append(before)
        log["psnr_after"].append(psnr(frame))
    s.initialize, s.map_frame, s._tracking_loss, s._mapping_loss = initialize, map_frame, tracking_loss, mapping_loss
    for frame in frames[:n_frames]:
        launched = len(counter.calls)
        s.step(frame)
        log["launches"].append(counter.calls[launched:])
        log["counts"].append(int(s.params["means3D"].shape[0]))
        log["rows"].append(_row_counts(s))
    ate = evaluate.trajectory_ate([f["gt_w2c"] for f in frames], s.estimated_w2c()) if n_frames == FRAMES else None      # whole runs only
    log["psnr_before"] = [float(x) for x in log["psnr_before"]]
    log["psnr_after"] = [float(x) for x in log["psnr_after"]]
    return s, log, ate


@pytest.fixture(scope="module")
def tracked(sequence):
    mp = pytest.MonkeyPatch()
    try:
        yield _run_session(sequence, 20, _ResampleCounter(mp))
    finally:
        mp.undo()


def test_tracking_runs_reduced_and_mapping_at_full_size(tracked):
    s, log, _ate = tracked
    small, full = (3, TH, TW), (3, H, W)
    print("slam_multires loss calls: tracking %d at %s, mapping %d at %s" % (len(log["tracking_shapes"]), small, len(log["mapping_shapes"]), full))
    assert s.num_tracking_iters == 20 and len(log["tracking_shapes"]) == 20 * (FRAMES - 1) and len(log["mapping_shapes"]) == 15 * FRAMES
    assert set(log["tracking_shapes"]) == {(small, small, (1, TH, TW), (1, TH, TW))}                    # condition 1
    assert set(log["mapping_shapes"]) == {(full, full, (1, H, W), (1, H, W))}
    assert len(s.keyframe_list) == 5
    for kf in s.keyframe_list:                                                                          # condition 2
        assert tuple(kf["color"].shape) == full and tuple(kf["depth"].shape) == (1, H, W) and kf["cam"] is s.cam
    assert (s.tracking_cam.image_height, s.tracking_cam.image_width) == (TH, TW) == (s.densify_cam.image_height, s.densify_cam.image_width)
    assert s.tracking_cam is not s.cam and s.densify_cam is not s.cam
    for f in ("bg", "scale_modifier", "sh_degree", "prefiltered", "debug"):      # what is not a matter of size is the given camera's
        assert getattr(s.tracking_cam, f) is getattr(s.cam, f) and getattr(s.densify_cam, f) is getattr(s.cam, f)
    k, tk = s.intrinsics.cpu(), s.tracking_intrinsics.cpu()
    assert torch.equal(tk, torch.tensor([[0.5, 1, 0.5], [1, 0.5, 0.5], [1, 1, 1]]) * k) and torch.equal(s.densify_intrinsics.cpu(), tk)
    assert set(s.variables["seen"].shape) == {log["counts"][-1]}


def test_one_resample_launch_per_frame(tracked):
    _s, log, _ate = tracked
    print("slam_multires resample launches per stepped frame: %s" % [len(c) for c in log["launches"]])
    assert log["launches"] == [[[(TH, TW)]]] * FRAMES              # condition 3: one call, one shared level (the two sizes are equal)


def test_tracking_lowers_the_trajectory_error(sequence, tracked, monkeypatch):
    _s0, _log0, ate_seeded = _run_session(sequence, 0, _ResampleCounter(monkeypatch))
    _s, _log, ate = tracked
    print("slam_multires ATE-RMSE [m]: 20 tracking iterations at %dx%d %.6f   pose seeding only %.6f" % (TW, TH, ate, ate_seeded))
    assert np.isfinite(ate) and ate < ate_seeded                  # condition 4


def test_first_frame_map_comes_from_the_densification_frame(sequence, monkeypatch):
    from hsr_utils import resample_frame, slam
    _cam, _k, frames = sequence
    s, log, _ate = _run_session(sequence, 20, _ResampleCounter(monkeypatch), n_frames=1)
    (small_im, small_depth), = resample_frame(frames[0]["im"], frames[0]["depth"], [(TH, TW)])
    positive = int((small_depth > 0).sum())
    print("slam_multires Gaussians after step(frame 0): %d (positive pixels of the %dx%d depth: %d; of the frame: %d)"
          % (log["counts"][0], TW, TH, positive, int((frames[0]["depth"] > 0).sum())))
    assert log["counts"][0] == positive == TH * TW                # condition 5: 6144 with full coverage, not 24576
    M, means, _rgb, log_scales, _rots, _opac, radius = slam.map_init_frame(small_im, small_depth, s.densify_intrinsics, torch.eye(4, device="cuda"), 3, 1)
    assert M == positive
    assert torch.equal(log["init"]["means3D"], means) and torch.equal(log["init"]["log_scales"], log_scales)      # condition 6
    assert torch.equal(s.variables["scene_radius"].reshape(1), radius)
    assert np.float32(float(radius)) == np.float32(float(small_depth.max())) * np.float32(1.0 / 3)      # :456, from the densification depth


def test_mapping_raises_the_last_frames_psnr(tracked):
    _s, log, _ate = tracked
    print("slam_multires full-resolution PSNR [dB] of frame %d: before its mapping step %.4f   after %.4f" % (FRAMES - 1, log["psnr_before"][-1], log["psnr_after"][-1]))
    print("slam_multires PSNR [dB] per frame before / after mapping: %s" % " ".join("%.2f/%.2f" % p for p in zip(log["psnr_before"], log["psnr_after"])))
    assert len(log["psnr_after"]) == FRAMES
    assert log["psnr_after"][-1] > log["psnr_before"][-1]         # condition 7


def test_row_counts_stay_consistent(tracked):
    _s, log, _ate = tracked
    print("slam_multires Gaussians after each step: %s" % log["counts"])
    for t, rows in enumerate(log["rows"]):                         # condition 8
        assert set(rows.values()) == {log["counts"][t]}, (t, rows)
        assert any(k.startswith("exp_avg_sq/") for k in rows)


def test_frame_sized_keys_share_the_camera_and_launch_nothing(sequence, monkeypatch):
    counter = _ResampleCounter(monkeypatch)
    s, log, _ate = _run_session(sequence, 3, counter, sizes=((H, W), (H, W)), n_frames=2)
    assert s.tracking_cam is s.cam and s.densify_cam is s.cam and s.tracking_intrinsics is s.intrinsics and s.densify_intrinsics is s.intrinsics
    assert counter.calls == [] and log["counts"][0] == H * W      # condition 9
    assert set(log["tracking_shapes"]) == {((3, H, W), (3, H, W), (1, H, W), (1, H, W))}
    data = s.tracking_data(sequence[2][1])
    assert data["im"] is sequence[2][1]["im"] and data["depth"] is sequence[2][1]["depth"] and data["cam"] is s.cam


def test_caller_supplied_tracking_tensors_take_precedence(sequence, monkeypatch):
    from hsr_utils import resample_frame
    _cam, _k, frames = sequence
    counter = _ResampleCounter(monkeypatch)
    constant = torch.full((3, TH, TW), 0.25, device="cuda")
    own = [dict(f) for f in frames[:2]]
    own[1]["tracking_im"] = constant
    own[1]["tracking_depth"] = resample_frame(frames[1]["im"], frames[1]["depth"], [(TH, TW)])[0][1]
    counter.calls.clear()
    keys = set(own[1])
    _s, log, _ate = _run_session(sequence, 4, counter, frames=own, n_frames=2)
    assert len(log["tracking_gt"]) == 4 and all(gt is constant for gt in log["tracking_gt"])      # condition 10
    assert log["launches"] == [[[(TH, TW)]], [[(TH, TW)]]]        # frame 1 still resamples once, for the densification level alone
    assert set(own[1]) == keys                                     # the caller's frame dict is not modified
    wrong = [dict(f) for f in frames[:2]]
    wrong[1]["tracking_im"], wrong[1]["tracking_depth"] = torch.zeros(3, TH, TW + 1, device="cuda"), own[1]["tracking_depth"]
    with pytest.raises(RuntimeError, match=r"'tracking_im' must be \[3,%d,%d\]" % (TH, TW)):
        _run_session(sequence, 4, counter, frames=wrong, n_frames=2)
    lone = [dict(f) for f in frames[:2]]
    lone[1]["tracking_im"] = constant
    with pytest.raises(RuntimeError, match=r"'tracking_depth' \[1,%d,%d\]" % (TH, TW)):
        _run_session(sequence, 4, counter, frames=lone, n_frames=2)
