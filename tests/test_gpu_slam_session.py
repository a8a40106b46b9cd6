"""GPU suite for hsr_utils.slam.SlamSession: a whole tracking-and-mapping run on a synthetic RGB-D sequence.

The sequence: 6 frames at 96x64 with K = 4 semantic planes in a 2-level tree (2 + 2 classes), rendered with the library's own semantic
forward from a hidden ground-truth map — hsr_utils.synthetic.make_scene's Gaussians (colours, semantics) moved onto a smooth wavy surface
2-3 m in front of the first camera and made near-opaque, so that the rendered depth is a surface a map can be built from — along a
smooth camera path of about half a pixel of image motion per frame.  The session is initialised from frame 0 (step(frame 0)) and stepped
through frames 1-5 with 20 tracking and 15 mapping iterations, map_every = 1, a window of 4, keyframe_every = 2; seeds fixed for torch,
numpy and random.  The tracking silhouette threshold is 0.9, not the reference's 0.99: 15 mapping iterations (the reference runs 60)
leave the first-frame map's opacity short of 0.99 over much of the image, and a mask that selects nothing tracks nothing.

Conditions (the figures are printed; the first MI355X run's are in profiles/slam_session_gpu.log):
  1. the session's ATE-RMSE (evaluate.trajectory_ate) is lower than that of the same session with 0 tracking iterations (pose seeding only);
  2. the PSNR (evaluate.frame_metrics) of the last frame is higher after its mapping step than before it;
  3. the Gaussian count after frame 1's densification is at least the count after initialisation, and after every step every per-Gaussian
     parameter, Adam moment and bookkeeping vector has the same row count;
  4. keyframe ids and every mapping window follow the rules pinned in tests/test_slam_cpu.py;
  5. a mapping step leaves the pose columns of the frames outside its window bit-unchanged."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

W, H, LEVELS, FRAMES = 96, 64, [2, 2], 6
K = sum(LEVELS)


def _intrinsics():
    from hsr_utils.camera import replica_intrinsics
    return replica_intrinsics(W, H)


def _gt_path():
    """world-to-camera of every frame relative to frame 0: a constant twist, ~0.5 px of image motion per frame at 2.5 m"""
    rots, trans = torch.zeros(1, 4, FRAMES), torch.zeros(1, 3, FRAMES)
    for t in range(FRAMES):
        q = torch.tensor([1.0, 0.0015 * t, -0.0030 * t, 0.0010 * t])
        rots[0, :, t] = q / q.norm()
        trans[0, :, t] = torch.tensor([0.018 * t, -0.008 * t, 0.012 * t])
    return rots, trans


def _hidden_map(kmat):
    from hsr_utils import make_scene
    P = 30000
    sc = make_scene(P, W, H, K, kmat, seed=7, kind="slam")
    fx, fy, cx, cy = kmat[0][0], kmat[1][1], kmat[0][2], kmat[1][2]
    g = torch.Generator().manual_seed(8)
    u = torch.rand(P, generator=g) * (W + 48) - 24
    v = torch.rand(P, generator=g) * (H + 48) - 24
    z = 2.5 + 0.35 * torch.sin(u / 9.0) + 0.25 * torch.cos(v / 7.0)
    means = torch.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], dim=1).float()
    colour = 0.5 + 0.25 * torch.stack([torch.sin(u / 5.0), torch.cos(v / 4.0), torch.sin((u + v) / 6.0)], dim=1) + 0.25 * (sc["colors_precomp"] - 0.5)
    sem = sc["semantics_precomp"].clone()
    sem[:, 0] += (u > W / 2).float()                                  # level 0 splits the image left / right,
    sem[:, 2] += (v > H / 2).float()                                  # level 1 top / bottom: label maps with structure
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


def _config(tracking_iters):
    zero = dict(means3D=0.0, rgb_colors=0.0, unnorm_rotations=0.0, logit_opacities=0.0, log_scales=0.0, semantic=0.0)
    return dict(
        num_frames=FRAMES, num_semantic=LEVELS, map_every=1, keyframe_every=2, mapping_window_size=4, scene_radius_depth_ratio=3,
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
        assert p is s.params[group["name"]]                        # the optimizer owns exactly the live parameters
        st = s.optimizer.state.get(p, {})
        for m in ("exp_avg", "exp_avg_sq"):
            if m in st:
                rows["%s/%s" % (m, group["name"])] = int(st[m].shape[0])
    return rows


def _run_session(sequence, tracking_iters):
    from hsr_utils import SlamSession, evaluate
    cam, intrinsics, frames = sequence
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    s = SlamSession(_config(tracking_iters), intrinsics, torch.eye(4, device="cuda"), cam)
    log = dict(psnr_before=[], psnr_after=[], windows=[], count_at_window=[], keyframes_at_window=[], rows=[], cams_unchanged=[])

    def psnr(frame):
        im, depth, _opac, _sem = s.render(frame["id"])
        return evaluate.frame_metrics(im, frame["im"], depth, frame["depth"])[0]

    window_of, map_of = s.mapping_window, s.map_frame

    def mapping_window(frame):                                      # runs right after the frame's densification
        log["count_at_window"].append(int(s.params["means3D"].shape[0]))
        log["keyframes_at_window"].append([kf["id"] for kf in s.keyframe_list])
        return window_of(frame)

    def map_frame(frame):
        before = psnr(frame)
        cams = {k: s.params[k].detach().clone() for k in ("cam_unnorm_rots", "cam_trans")}
        map_of(frame)
        outside = [t for t in range(FRAMES) if t not in s.last_window[0]]
        log["cams_unchanged"].append(all(torch.equal(s.params[k].detach()[..., outside], cams[k][..., outside]) for k in cams))
        log["psnr_before"].append(before)
        log["psnr_after"].append(psnr(frame))
        log["windows"].append(s.last_window)
    s.mapping_window, s.map_frame = mapping_window, map_frame
    counts = []
    for frame in frames:
        s.step(frame)
        counts.append(int(s.params["means3D"].shape[0]))
        log["rows"].append(_row_counts(s))
    ate = evaluate.trajectory_ate([f["gt_w2c"] for f in frames], s.estimated_w2c())
    log["psnr_before"] = [float(x) for x in log["psnr_before"]]      # read once, at the end
    log["psnr_after"] = [float(x) for x in log["psnr_after"]]
    return s, log, counts, ate


@pytest.fixture(scope="module")
def tracked(sequence):
    return _run_session(sequence, 20)


def test_tracking_lowers_the_trajectory_error(sequence, tracked):
    _s0, _log0, _counts0, ate_seeded = _run_session(sequence, 0)
    s, _log, _counts, ate = tracked
    print("slam_session ATE-RMSE [m]: 20 tracking iterations %.6f   pose seeding only %.6f" % (ate, ate_seeded))
    assert s.num_tracking_iters == 20
    assert np.isfinite(ate) and ate < ate_seeded


def test_mapping_raises_the_last_frames_psnr(tracked):
    _s, log, _counts, _ate = tracked
    print("slam_session PSNR [dB] of frame %d: before its mapping step %.4f   after %.4f" % (FRAMES - 1, log["psnr_before"][-1], log["psnr_after"][-1]))
    print("slam_session PSNR [dB] per frame before / after mapping: %s" % " ".join("%.2f/%.2f" % p for p in zip(log["psnr_before"], log["psnr_after"])))
    assert len(log["psnr_after"]) == FRAMES                         # map_every = 1: every frame was mapped
    assert log["psnr_after"][-1] > log["psnr_before"][-1]


def test_row_counts_stay_consistent(tracked):
    s, log, counts, _ate = tracked
    initial = counts[0]
    print("slam_session Gaussians: after initialisation %d, after frame 1's densification %d, after each step %s"
          % (initial, log["count_at_window"][1], counts))
    assert 0 < initial <= W * H
    assert log["count_at_window"][0] == initial                     # frame 0 is mapped without densification
    assert log["count_at_window"][1] >= initial
    for t, rows in enumerate(log["rows"]):
        assert set(rows.values()) == {counts[t]}, (t, rows)
        assert any(k.startswith("exp_avg_sq/") for k in rows)       # the moments were there to be counted
    assert int(s.variables["timestep"].max()) <= FRAMES - 1


def test_keyframes_and_windows_follow_the_rules(tracked):
    s, log, _counts, _ate = tracked
    assert s.keyframe_time_indices == [0, 1, 3, 4, 5] == [kf["id"] for kf in s.keyframe_list]      # keyframe_every 2, 6 frames
    assert [list(k) for k in log["keyframes_at_window"]] == [[], [0], [0, 1], [0, 1], [0, 1, 3], [0, 1, 3, 4]]
    for t, ((time_idx, window), kf_ids) in enumerate(zip(log["windows"], log["keyframes_at_window"])):
        assert window[-1] == -1 and time_idx[-1] == t               # the current frame closes the window
        body, body_ids = [int(i) for i in window[:-1]], time_idx[:-1]
        if kf_ids:
            assert body[-1] == len(kf_ids) - 1 and body_ids[-1] == kf_ids[-1]      # the last keyframe before it
            chosen = body[:-1]
            assert len(chosen) <= 2 and len(set(chosen)) == len(chosen) and all(0 <= i < len(kf_ids) - 1 for i in chosen)
            assert body_ids[:-1] == [kf_ids[i] for i in chosen]
        else:
            assert body == []
        assert len(window) <= 4


def test_mapping_leaves_other_frames_poses_alone(tracked):
    _s, log, _counts, _ate = tracked
    assert len(log["cams_unchanged"]) == FRAMES and all(log["cams_unchanged"])
