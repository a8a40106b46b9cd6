"""GPU suite for hsr_utils.slam.SlamSession with ignore_outlier_depth_loss = True in the tracking and the mapping section: the session's
losses go through the fused outlier-rejecting head (include/ext/hsr_loss_outlier.h), once per iteration.

The sequence and the config are those of tests/test_gpu_slam_session.py (96x64, K = 4 semantic planes in a 2-level tree, a hidden map on a
wavy surface, half a pixel of image motion per frame), cut to 3 frames with 6 tracking and 5 mapping iterations.  Conditions:
  1. hsr_loss_outlier_value is called once per tracking and once per mapping iteration (2 * 6 + 3 * 5 calls);
  2. every parameter and Adam moment is finite, and the row counts of parameters, moments and bookkeeping agree after every step;
  3. on the last frame's render, session._tracking_loss and session._mapping_loss equal the eager composition they replace (_outlier_mask +
     masked_l1 + weighted_sum) on the same tensors: totals within VAL_TOL of tests/test_gpu_losses.py, gradients w.r.t. the rendered image and
     depth bit-equal for the tracking sums and within 1 ulp for the mapping mean.
No ATE or PSNR threshold: none has been measured with the flag on."""
import random

import numpy as np
import pytest
import torch

from test_gpu_losses import VAL_TOL

pytestmark = pytest.mark.gpu

W, H, LEVELS, FRAMES = 96, 64, [2, 2], 3
K = sum(LEVELS)
TRACK_ITERS, MAP_ITERS = 6, 5


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
    sem[:, 0] += (u > W / 2).float()
    sem[:, 2] += (v > H / 2).float()
    scale = (1.3 * z / (0.5 * (fx + fy))).float()
    return {"means3D": means, "rgb_colors": colour.float().clamp(0, 1), "unnorm_rotations": sc["rotations"],
            "logit_opacities": torch.full((P, 1), 3.0), "log_scales": scale.log()[:, None], "semantic": sem}


@pytest.fixture(scope="module")
def sequence():
    from diff_gaussian_rasterization import GaussianRasterizer_semantic
    from hsr_utils import setup_camera, slam, slam_helpers as SH
    from hsr_utils.camera import replica_intrinsics
    kmat = replica_intrinsics(W, H)
    cam = setup_camera(W, H, kmat, np.eye(4), device="cuda")
    hidden = {k: v.cuda().contiguous() for k, v in _hidden_map(kmat).items()}
    rots, trans = _gt_path()
    hidden["cam_unnorm_rots"], hidden["cam_trans"] = rots.cuda(), trans.cuda()
    frames = []
    with torch.no_grad():
        for t in range(FRAMES):
            rv = SH.transformed_params2rendervar_semantic(hidden, SH.transform_to_frame(hidden, t, False, False))
            im, _radius, sem, depth, _median, _opac = GaussianRasterizer_semantic(raster_settings=cam)(**rv)
            labels = torch.stack([sem[:2].argmax(dim=0), sem[2:4].argmax(dim=0)])
            frames.append({"id": t, "im": im.clamp(0, 1).contiguous(), "depth": depth.contiguous(), "semantic_label_gt": labels,
                           "gt_w2c": slam.frame_w2c(hidden, t)})
    return cam, torch.tensor(kmat, dtype=torch.float32, device="cuda"), frames


def _config():
    zero = dict(means3D=0.0, rgb_colors=0.0, unnorm_rotations=0.0, logit_opacities=0.0, log_scales=0.0, semantic=0.0)
    return dict(
        num_frames=FRAMES, num_semantic=LEVELS, map_every=1, keyframe_every=2, mapping_window_size=4, scene_radius_depth_ratio=3,
        mean_sq_dist_method="projective", gaussian_distribution="isotropic",
        tracking=dict(num_iters=TRACK_ITERS, use_gt_poses=False, forward_prop=True, use_sil_for_loss=True, sil_thres=0.9, use_l1=True,
                      ignore_outlier_depth_loss=True, loss_weights=dict(im=0.5, depth=1.0),
                      lrs=dict(zero, cam_unnorm_rots=4e-4, cam_trans=2e-3)),
        mapping=dict(num_iters=MAP_ITERS, add_new_gaussians=True, sil_thres=0.5, use_l1=True, use_sil_for_loss=False, ignore_outlier_depth_loss=True,
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
    finite = all(bool(torch.isfinite(p).all()) for p in s.params.values())
    for group in s.optimizer.param_groups:
        p = group["params"][0]
        st = s.optimizer.state.get(p, {})
        for m in ("exp_avg", "exp_avg_sq"):
            if m in st:
                finite = finite and bool(torch.isfinite(st[m]).all())
                if group["name"] not in SE.CAMERA_KEYS:
                    rows["%s/%s" % (m, group["name"])] = int(st[m].shape[0])
    return rows, finite


@pytest.fixture(scope="module")
def stepped(sequence):
    """the session after three frames, with a spy on the fused entry point"""
    from diff_gaussian_rasterization import _abi
    from hsr_utils import SlamSession
    cam, intrinsics, frames = sequence
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    calls = {"outlier": 0, "tracking": 0}
    real_outlier, real_tracking = _abi.lib.hsr_loss_outlier_value, _abi.lib.hsr_loss_tracking_value

    def spy_outlier(*args):
        calls["outlier"] += 1
        return real_outlier(*args)

    def spy_tracking(*args):
        calls["tracking"] += 1
        return real_tracking(*args)
    _abi.lib.hsr_loss_outlier_value, _abi.lib.hsr_loss_tracking_value = spy_outlier, spy_tracking
    try:
        s = SlamSession(_config(), intrinsics, torch.eye(4, device="cuda"), cam)
        rows, iters = [], []
        for frame in frames:
            s.step(frame)
            rows.append(_row_counts(s))
            iters.append(s.num_tracking_iters)
    finally:
        _abi.lib.hsr_loss_outlier_value, _abi.lib.hsr_loss_tracking_value = real_outlier, real_tracking
    return s, frames, dict(calls), rows, iters


def test_the_fused_head_runs_once_per_iteration(stepped):
    _s, _frames, calls, _rows, iters = stepped
    assert iters == [0] + [TRACK_ITERS] * (FRAMES - 1)
    assert calls == {"outlier": (FRAMES - 1) * TRACK_ITERS + FRAMES * MAP_ITERS, "tracking": 0}


def test_state_stays_finite_and_row_counts_agree(stepped):
    s, _frames, _calls, rows, _iters = stepped
    for t, (counts, finite) in enumerate(rows):
        assert finite, t
        assert len(set(counts.values())) == 1 and any(k.startswith("exp_avg_sq/") for k in counts), (t, counts)
    assert rows[-1][0]["means3D"] == int(s.params["means3D"].shape[0]) > 0


def _ulps(a, b):
    def ordered(t):
        i = t.detach().cpu().reshape(-1).view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7fffffff), i)
    return int((ordered(a) - ordered(b)).abs().max())


def test_session_losses_equal_the_eager_composition(stepped):
    from hsr_utils import losses as L, slam
    s, frames, _calls, _rows, _iters = stepped
    frame = frames[-1]
    im0, depth0, opac, sem = s.render(frame["id"])
    trk, mp = s.config["tracking"], s.config["mapping"]
    mask = s._outlier_mask(frame["depth"], depth0)
    tmask = mask & (opac > trk["sil_thres"])
    assert int(tmask.sum()) > 0                                    # there is a selection to compare on

    def leaves():
        return im0.clone().requires_grad_(True), depth0.clone().requires_grad_(True)

    # tracking: sums
    im, depth = leaves()
    loss, parts = s._tracking_loss(frame, im, depth, opac)
    loss.backward()
    loss = loss.detach()
    im_e, depth_e = leaves()
    d = L.masked_l1(depth_e, frame["depth"], tmask, "sum")
    c = L.masked_l1(im_e, frame["im"], tmask, "sum")
    eager = L.weighted_sum((d, c), (trk["loss_weights"]["depth"], trk["loss_weights"]["im"]))
    eager.backward()
    eager = eager.detach()
    dist = abs(float(loss) - float(eager)) / abs(float(eager))
    print("slam_session_outlier tracking: %d of %d pixels selected; fused total %.9g eager %.9g (relative distance %.3g)"
          % (int(tmask.sum()), tmask.numel(), float(loss), float(eager), dist))
    assert dist <= VAL_TOL
    assert abs(float(parts[0]) - float(d)) <= VAL_TOL * abs(float(d)) and abs(float(parts[1]) - float(c)) <= VAL_TOL * abs(float(c))
    assert torch.equal(im.grad, im_e.grad) and torch.equal(depth.grad, depth_e.grad)
    assert not depth.grad[~tmask.reshape(depth.shape)].any() and depth.grad.any()

    # mapping: the depth term is a mean over the outlier-rejecting mask; the other heads are the same calls on both sides
    im, depth = leaves()
    loss = s._mapping_loss(frame, im, sem, depth, 0)
    loss.backward()
    loss = loss.detach()
    im_e, depth_e = leaves()
    d = L.masked_l1(depth_e, frame["depth"], mask, "mean")
    terms, weights = [d, L.mapping_image_loss(im_e, frame["im"])], [mp["loss_weights"]["depth"], mp["loss_weights"]["im"]]
    H_, W_ = sem.shape[-2:]
    assert list(s.level_sizes) == LEVELS and s.mlp is None          # iteration 0 of this config: the tree head alone
    terms.append(L.tree_cross_entropy(sem, frame["semantic_label_gt"].reshape(-1, H_, W_)[:len(LEVELS)], s.level_sizes,
                                      [slam.WEIGHT_SEM[0]] * len(LEVELS)))
    weights.append(mp["loss_weights"]["sem"])
    eager = L.weighted_sum(terms, weights)
    eager.backward()
    eager = eager.detach()
    dist = abs(float(loss) - float(eager)) / abs(float(eager))
    ulps = _ulps(depth.grad, depth_e.grad)
    print("slam_session_outlier mapping: %d of %d pixels selected; fused total %.9g eager %.9g (relative distance %.3g); depth gradient off by %d ulp"
          % (int(mask.sum()), mask.numel(), float(loss), float(eager), dist, ulps))
    assert dist <= VAL_TOL
    assert ulps <= 1 and torch.equal(im.grad, im_e.grad)
    assert not depth.grad[~mask.reshape(depth.shape)].any() and depth.grad.any()
