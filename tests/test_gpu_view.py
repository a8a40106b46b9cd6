"""GPU suite for the novel-view path (include/ext/hsr_view.h): hsr_view_prep against the restatements of tests/view_ref.py and, bit for
bit, against the frame path for equal matrices; hsr_view_holes against numpy; render_view against the rasterizer called by hand on
hsr_view_prep's outputs; and evaluate_novel_views on a small synthetic map with one view turned away."""
import os

import numpy as np
import pytest
import torch

import view_ref as R
from test_view_cpu import _rot

pytestmark = pytest.mark.gpu

FWD_RTOL, FWD_ATOL = 2e-6, 2e-6      # tests/test_gpu_frame_prep.py's forward bounds: the same expressions, libm-vs-device exp / sqrt ulps
PSNR_TOL, DEPTH_TOL = 1e-4, 2e-6     # tests/test_gpu_eval.py's bounds of frame_metrics against float64
CANARY = 12345.0
OUTPUTS = (("means3D", 3), ("unnorm_rotations", 4), ("rotations", 4), ("opacities", 1), ("scales", 3))


def _w2c(rotation, translation):
    m = np.eye(4, dtype=np.float64)
    m[:3, :3], m[:3, 3] = rotation, translation
    return m.astype(np.float32)


# identity, a tilted camera, and one matrix per pivot branch of the quaternion (0: small angle; 1, 2, 3: near half turns about x, y, z)
MATRICES = [
    ("identity", np.eye(4, dtype=np.float32), 0),
    ("tilted", _w2c(_rot([0.9, 0.2, -0.1], 23.0), (0.3, -0.2, 0.5)), 0),
    ("branch w", _w2c(_rot([-0.2, 0.4, 0.9], 61.0), (-1.0, 0.25, 0.0)), 0),
    ("branch x", _w2c(_rot([0.95, 0.1, -0.2], 172.0), (0.1, 0.2, -0.3)), 1),
    ("branch y", _w2c(_rot([0.15, -0.97, 0.1], 168.0), (2.0, 0.0, 1.0)), 2),
    ("branch z", _w2c(_rot([0.3, -0.5, 0.81], 171.0), (0.0, -0.7, 0.4)), 3),
]


def _inputs(P, S, seed):
    g = np.random.default_rng(seed)
    p = {"means3D": (g.standard_normal((P, 3)) * 3).astype(np.float32), "unnorm_rotations": g.standard_normal((P, 4)).astype(np.float32),
         "logit_opacities": (g.standard_normal((P, 1)) * 2).astype(np.float32), "log_scales": (g.standard_normal((P, S)) - 3).astype(np.float32)}
    if P > 3:      # F.normalize's clamp: rows of zeros and one of norm 1e-20
        p["unnorm_rotations"][1] = 0
        p["unnorm_rotations"][P // 2] = 0
        p["unnorm_rotations"][2] = (6e-21, -8e-21, 0, 0)
    return p


def _view_prep(dev_in, w2c, S, transform_rots, rot_source, with_unnorm=True):
    """hsr_view_prep through the C ABI into canary-guarded buffers; returns the outputs as [P,c] tensors"""
    from diff_gaussian_rasterization import _abi
    P = dev_in["means3D"].shape[0]
    bufs = {k: torch.full((P * c + 64,), CANARY, device="cuda") for k, c in OUTPUTS}
    ptr = lambda t: t.data_ptr() if t.numel() else None
    _abi.call(_abi.lib.hsr_view_prep, "hsr_view_prep", torch.device("cuda", torch.cuda.current_device()), P, S, int(transform_rots), rot_source,
              ptr(dev_in["means3D"]), ptr(dev_in["unnorm_rotations"]), ptr(dev_in["logit_opacities"]), ptr(dev_in["log_scales"]), w2c.data_ptr(),
              bufs["means3D"].data_ptr(), bufs["unnorm_rotations"].data_ptr() if with_unnorm else None, bufs["rotations"].data_ptr(),
              bufs["opacities"].data_ptr(), bufs["scales"].data_ptr())
    out = {}
    for k, c in OUTPUTS:
        assert (bufs[k][P * c:] == CANARY).all(), "%s: written past row P" % k
        out[k] = bufs[k][:P * c].view(P, c)
    if not with_unnorm:
        assert (out.pop("unnorm_rotations") == CANARY).all()
    return out


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("P", [0, 1, 255, 256, 257, 1000])
def test_view_prep_matches_the_restatements(P, S):
    inp = _inputs(P, S, 10 * P + S)
    dev_in = {k: torch.tensor(v, device="cuda") for k, v in inp.items()}
    for name, w2c, branch in MATRICES:
        m = torch.tensor(w2c[:3, :3])
        pivots = torch.stack([1 + m[0, 0] + m[1, 1] + m[2, 2], 1 + m[0, 0] - m[1, 1] - m[2, 2], 1 - m[0, 0] + m[1, 1] - m[2, 2],
                              1 - m[0, 0] - m[1, 1] + m[2, 2]])
        assert int(pivots.argmax()) == branch, name
        w2c_dev = torch.tensor(w2c, device="cuda")
        bound = R.means_bound(inp, w2c)
        for transform_rots in (False, True):
            for rot_source in (R.ROT_PARAMS, R.ROT_TRANSFORMED):
                got = {k: v.cpu().numpy() for k, v in _view_prep(dev_in, w2c_dev, S, transform_rots, rot_source).items()}
                f64 = R.transform(inp, w2c, rot_source, torch.float64, transform_rots)
                f32 = R.transform(inp, w2c, rot_source, torch.float32, transform_rots)
                what = (name, transform_rots, rot_source)
                assert got["means3D"].shape == (P, 3) and (np.abs(got["means3D"].astype(np.float64) - f64["means3D"]) <= bound).all(), what
                for k in ("unnorm_rotations", "rotations", "opacities", "scales"):
                    assert got[k].dtype == np.float32 and got[k].shape == f32[k].shape, (k, what)
                    np.testing.assert_allclose(got[k], f32[k], rtol=FWD_RTOL, atol=FWD_ATOL, err_msg="%s %s" % (k, what))
                    np.testing.assert_allclose(got[k], f64[k], rtol=2 * FWD_RTOL, atol=2 * FWD_ATOL, err_msg="%s %s float64" % (k, what))
                if name == "identity":
                    assert np.array_equal(got["means3D"].view(np.uint32), inp["means3D"].view(np.uint32)), what
                if not transform_rots:
                    assert np.array_equal(got["unnorm_rotations"].view(np.uint32), inp["unnorm_rotations"].view(np.uint32)), what
                if P > 3:      # the clamp of F.normalize: a zero row stays zero, through the quaternion product too
                    assert not got["rotations"][1].any() and np.isfinite(got["rotations"]).all() and np.isfinite(got["unnorm_rotations"]).all()
    if P:      # out_unnorm_rot may be NULL: the other outputs are the same
        w2c_dev = torch.tensor(MATRICES[1][1], device="cuda")
        a = _view_prep(dev_in, w2c_dev, S, S == 3, R.ROT_TRANSFORMED)
        b = _view_prep(dev_in, w2c_dev, S, S == 3, R.ROT_TRANSFORMED, with_unnorm=False)
        assert all(torch.equal(a[k], b[k]) for k in b)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("quaternion", [(1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, -1.0, 0.0), (0.0, 0.0, 0.0, 1.0)])
def test_means_equal_the_frame_paths_bit_for_bit_for_equal_matrices(quaternion, S):
    """a unit-norm, axis-aligned pose quaternion makes the frame kernel's R exact (entries 0, 1, -1), so the twelve floats it forms can be
    written down: with them as w2c, hsr_view_prep gives the bits hsr_frame_prep_forward gives"""
    from hsr_utils import slam, slam_helpers as SH
    P, frames, t = 1000, 3, 1
    params = {k: torch.tensor(v, device="cuda") for k, v in _inputs(P, S, 77).items()}
    params["rgb_colors"] = torch.rand(P, 3, device="cuda")
    params["cam_unnorm_rots"] = torch.zeros(1, 4, frames, device="cuda")
    params["cam_unnorm_rots"][0, 0, :] = 1
    params["cam_unnorm_rots"][0, :, t] = torch.tensor(quaternion)
    params["cam_trans"] = torch.tensor([[0.0, 0.37, 0.0], [0.0, -1.25, 0.0], [0.0, 0.0625 + 1e-3, 0.0]], device="cuda").reshape(1, 3, frames)
    with torch.no_grad():
        w2c = slam.frame_w2c(params, t)
        assert sorted(set(w2c[:3, :3].abs().flatten().tolist())) == [0.0, 1.0] and torch.equal(w2c[:3, 3], params["cam_trans"][0, :, t])
        frame = SH.transform_to_frame(params, t, False, False)
        view = SH.transform_to_view(params, w2c)
        rv_f, rv_v = SH.transformed_params2rendervar(params, frame), SH.transformed_params2rendervar(params, view)
    assert torch.equal(rv_f["means3D"].view(torch.int32), rv_v["means3D"].view(torch.int32))
    assert torch.equal(frame["means3D"], view["means3D"]) and view["means3D"] is rv_v["means3D"] and list(view.keys()) == ["means3D", "unnorm_rotations"]
    # the same expressions on the same inputs.  The camera quaternion is exact here too, up to its sign: the matrix gives the one with a
    # real part that is not negative, and -q is the same rotation (every product and quotient changes its sign exactly)
    for k, a, b in [(k, rv_f[k], rv_v[k]) for k in ("rotations", "opacities", "scales")] + [("unnorm", frame["unnorm_rotations"], view["unnorm_rotations"])]:
        assert torch.equal(a, b) or (S == 3 and k in ("rotations", "unnorm") and torch.equal(a, -b)), k
    assert not rv_v["means3D"].requires_grad and rv_v["colors_precomp"] is params["rgb_colors"]


# ---- the hole counts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (37, 53), (300, 421)])
def test_view_holes_equal_numpys_counts(H, W):
    from diff_gaussian_rasterization import _abi
    from hsr_utils import evaluate
    thres = np.float32(0.6)
    g = np.random.default_rng(H * W)
    sil = g.random((1, H, W)).astype(np.float32)
    special = np.array([thres, np.nextafter(thres, np.float32(1)), np.nextafter(thres, np.float32(0)), np.nan, np.inf, -np.inf, 0.0, 1.0], np.float32)
    pick = g.random((1, H, W)) < 0.5
    sil[pick] = special[g.integers(0, len(special), size=int(pick.sum()))]
    depth = (g.random((1, H, W)) * 4 + 0.1).astype(np.float32)
    kinds = g.integers(0, 6, size=(1, H, W))
    depth[kinds == 0] = 0
    depth[kinds == 1] = -1.5
    depth[kinds == 2] = np.nan
    cases = [(sil, depth)]
    if H * W == 1:      # every special value on the one pixel, with a valid and an invalid depth
        cases = [(np.full((1, 1, 1), s, np.float32), np.full((1, 1, 1), d, np.float32)) for s in special for d in (2.0, 0.0, -1.0, np.nan)]
    for s, d in cases:
        want = R.hole_counts(s, d, thres)
        s_dev, d_dev = torch.tensor(s, device="cuda"), torch.tensor(d, device="cuda")
        got = evaluate.view_holes(s_dev, d_dev, float(thres))
        assert got.dtype == torch.int64 and got.shape == (2,) and tuple(got.tolist()) == want, (H, W, got.tolist(), want)
        assert tuple(evaluate.view_holes(s_dev[0], d_dev[0], float(thres)).tolist()) == want      # [H,W] planes
    if H * W > 1:
        assert 0 < want[0] < want[1] < H * W
    # a second call into the same out2 overwrites it: nothing is accumulated, the caller clears nothing
    out = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    sc = torch.empty(int(_abi.lib.hsr_view_holes_scratch_bytes(H, W)), dtype=torch.uint8, device="cuda")
    dev = torch.device("cuda", torch.cuda.current_device())
    for _ in range(2):
        _abi.call(_abi.lib.hsr_view_holes, "hsr_view_holes", dev, H, W, s_dev.data_ptr(), d_dev.data_ptr(), float(thres), out.data_ptr(),
                  sc.data_ptr(), sc.numel())
        assert out.tolist() == [want[0], want[1], -7]
    ones = torch.ones(1, H, W, device="cuda")
    assert evaluate.view_holes(ones, ones, 2.0).tolist() == [H * W, H * W] and evaluate.view_holes(ones, ones, 0.5).tolist() == [0, H * W]


# ---- render_view ---------------------------------------------------------------------------------------------------------------------------
W_IMG, H_IMG = 64, 48


def _kmat():
    from hsr_utils.camera import replica_intrinsics
    return replica_intrinsics(W_IMG, H_IMG)


def _map(P=2500, S=1, K=0, seed=3):
    """a surface of about P Gaussians that covers the 64x48 image and a margin of 40 pixels around it, so that a camera moved a little
    still sees no hole (hsr_utils.synthetic for colours, rotations and semantic rows)"""
    from hsr_utils import make_scene
    kmat = _kmat()
    sc = make_scene(P, W_IMG, H_IMG, K, kmat, seed=seed, kind="slam" if S == 1 else "aniso")
    fx, fy, cx, cy = kmat[0][0], kmat[1][1], kmat[0][2], kmat[1][2]
    g = torch.Generator().manual_seed(seed + 1)
    u = torch.rand(P, generator=g) * (W_IMG + 80) - 40
    v = torch.rand(P, generator=g) * (H_IMG + 80) - 40
    z = 2.5 + 0.3 * torch.sin(u / 15.0) + 0.2 * torch.cos(v / 11.0)
    means = torch.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], dim=1).float()
    colour = (0.5 + 0.3 * torch.stack([torch.sin(u / 9.0), torch.cos(v / 7.0), torch.sin((u + v) / 11.0)], dim=1) + 0.2 * (sc["colors_precomp"] - 0.5))
    scale = (4.0 * z / (0.5 * (fx + fy))).float()
    log_scales = scale.log()[:, None] if S == 1 else (scale[:, None] * torch.tensor([1.0, 1.3, 0.8])).log()
    m = {"means3D": means, "rgb_colors": colour.float().clamp(0, 1), "unnorm_rotations": sc["rotations"] * 1.7,
         "logit_opacities": torch.full((P, 1), 3.0), "log_scales": log_scales.float()}
    if K:
        m["semantic"] = sc["semantics_precomp"]
    return {k: v.cuda().contiguous() for k, v in m.items()}


def _cam():
    from hsr_utils import setup_camera
    return setup_camera(W_IMG, H_IMG, _kmat(), np.eye(4), device="cuda")


@pytest.mark.parametrize("S,semantic", [(1, False), (3, False), (1, True), (3, True)])
def test_render_view_is_the_rasterizer_on_view_preps_outputs(S, semantic):
    import hsr_utils
    from diff_gaussian_rasterization import GaussianRasterizer, GaussianRasterizer_semantic
    params, cam = _map(S=S, K=6 if semantic else 0), _cam()
    w2c = MATRICES[1][1].copy()
    w2c[:3, 3] = (0.05, -0.03, 0.1)
    w2c[:3, :3] = _rot([0.1, 1.0, 0.2], 4.0)
    rv, im, radius, sem, depth, opac = hsr_utils.render_view(params, w2c, cam, semantic)      # a host matrix: copied once
    assert (sem is None) == (not semantic) and not im.requires_grad and float(opac.max()) > 0.9 and int((radius > 0).sum()) > 500
    prep = _view_prep(params, torch.tensor(w2c, device="cuda"), S, S == 3, R.ROT_PARAMS if semantic else R.ROT_TRANSFORMED)
    for k in ("means3D", "rotations", "opacities", "scales"):
        assert torch.equal(rv[k], prep[k].view_as(rv[k])), k
    hand = dict(means3D=prep["means3D"].contiguous(), means2D=torch.zeros_like(prep["means3D"]), colors_precomp=params["rgb_colors"],
                rotations=prep["rotations"].contiguous(), opacities=prep["opacities"].contiguous(), scales=prep["scales"].contiguous())
    with torch.no_grad():
        if semantic:
            im2, radius2, sem2, depth2, _median, opac2 = GaussianRasterizer_semantic(raster_settings=cam)(semantics_precomp=params["semantic"], **hand)
            assert torch.equal(sem, sem2)
        else:
            im2, radius2, depth2, _median, opac2, _mask = GaussianRasterizer(raster_settings=cam)(**hand)
    assert torch.equal(im, im2) and torch.equal(radius, radius2) and torch.equal(depth, depth2) and torch.equal(opac, opac2)
    # a device matrix is used as it is, a float64 one is converted: the same picture
    for other in (torch.tensor(w2c, device="cuda"), torch.tensor(w2c, dtype=torch.float64), w2c.astype(np.float64)):
        assert torch.equal(hsr_utils.render_view(params, other, cam, semantic)[1], im)


CONFIG = dict(tracking=dict(num_iters=1, lrs={}, loss_weights=dict(im=0.5, depth=1.0), sil_thres=0.99),
              mapping=dict(num_iters=1, lrs={}, loss_weights=dict(im=0.5, depth=1.0), sil_thres=0.5),
              map_every=1, keyframe_every=5, mapping_window_size=3, num_frames=3)


@pytest.mark.parametrize("S,semantic", [(1, False), (3, False), (1, True)])
def test_session_render_view_with_the_identity_equals_render_of_frame_0(S, semantic):
    from hsr_utils import SlamSession
    cam = _cam()
    cfg = dict(CONFIG, num_semantic=6) if semantic else CONFIG
    s = SlamSession(cfg, torch.tensor(_kmat(), dtype=torch.float32, device="cuda"), torch.eye(4, device="cuda"), cam)
    with pytest.raises(RuntimeError, match="before the first frame"):
        s.render_view(torch.eye(4))
    s.params = _map(S=S, K=6 if semantic else 0)
    s.params["cam_unnorm_rots"] = torch.tensor([1.0, 0.0, 0.0, 0.0], device="cuda").reshape(1, 4, 1).repeat(1, 1, 3).contiguous()
    s.params["cam_trans"] = torch.zeros(1, 3, 3, device="cuda")
    a, b = s.render(0), s.render_view(torch.eye(4, device="cuda"))
    assert len(a) == len(b) == 4 and (b[3] is None) == (not semantic)
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y)
    assert float(b[2].max()) > 0.9


# ---- evaluate_novel_views ------------------------------------------------------------------------------------------------------------------
SIL = 0.5
# the test views, relative to the training frame: two near it, one turned away by 30 degrees (a third of the image sees no map), one closer
VIEWS = [_w2c(np.eye(3), (0.06, 0.0, 0.0)), _w2c(_rot([0.0, 1.0, 0.0], 2.0), (0.0, 0.03, 0.0)), _w2c(_rot([0.0, 1.0, 0.0], 30.0), (0.0, 0.0, 0.0)),
         _w2c(_rot([1.0, 0.0, 0.0], -1.5), (0.0, 0.0, -0.1))]


@pytest.fixture(scope="module")
def nvs():
    """(params, camera, the five frames: the training frame and four test views, the renders of the test views as numpy)"""
    import hsr_utils
    params, cam = _map(), _cam()
    frames, renders = [], []
    for i, w2c in enumerate([np.eye(4, dtype=np.float32)] + VIEWS):
        _rv, im, _radius, _sem, depth, opac = hsr_utils.render_view(params, w2c, cam, False)
        gt_im = (im * 0.9).contiguous()                                   # PSNR stays finite
        gt_depth = torch.where(depth > 0, depth * 1.01, torch.full_like(depth, 2.0))      # the sensor sees a surface where the map has none
        if i == 2:
            gt_depth[:, 10:20, 30:50] = 0                                 # a block without depth
        frames.append({"im": gt_im, "depth": gt_depth.contiguous(), "gt_w2c": torch.tensor(w2c) if i % 2 else torch.tensor(w2c, device="cuda")})
        if i > 0:
            renders.append(tuple(t.cpu().numpy() for t in (im, depth, opac, gt_im, gt_depth)))
    return params, cam, frames, renders


def _check_scores(result, want, rows):
    for k, tol in (("psnr", PSNR_TOL), ("depth_l1", None), ("depth_rmse", None)):
        got, exp = result[k], want[k][rows]
        assert got.dtype == np.float64 and got.shape == exp.shape and np.isfinite(got).all(), k
        print(k, got, exp)
        assert (np.abs(got - exp) < tol).all() if tol else (np.abs(got - exp) <= DEPTH_TOL * np.abs(exp)).all(), (k, got, exp)


def test_evaluate_novel_views_scores_validity_files_and_pictures(nvs, tmp_path):
    from PIL import Image
    from hsr_utils import evaluate, export
    params, cam, frames, renders = nvs
    eval_dir = str(tmp_path / "nvs")
    result = evaluate.evaluate_novel_views(params, (f for f in frames), cam, eval_dir, sil_thres=SIL, mapping_iters=30, add_new_gaussians=True,
                                           save_frames=True, ms_ssim=False)
    want = R.nvs_loop(renders, SIL, 30, True)
    counts = [R.hole_counts(r[2], r[4], SIL) for r in renders]
    print("holes", result["holes"], result["percent_holes"], counts)
    assert result["frame_ids"] == [0, 1, 2, 3]
    assert result["holes"].dtype == np.int64 and result["holes"].tolist() == [c[0] for c in counts] == want["holes"].tolist()
    assert result["valid_depth"].tolist() == [c[1] for c in counts] and counts[1][1] == W_IMG * H_IMG - 200
    assert result["valid_nvs_frames"].dtype == np.bool_ and result["valid_nvs_frames"].tolist() == [True, True, False, True] == want["valid_nvs_frames"].tolist()
    assert result["percent_holes"].dtype == np.float32 and result["percent_holes"][2] > 1.0
    assert np.array_equal(result["percent_holes"], (result["holes"].astype(np.float32) / np.float32(W_IMG * H_IMG) * np.float32(100)))
    _check_scores(result, want, slice(None))
    valid = result["valid_nvs_frames"]
    for k in ("psnr", "depth_l1", "depth_rmse"):
        assert result["avg_" + k] == float(result[k][valid].mean()) and result["avg_" + k] != float(result[k].mean())
        assert abs(result["avg_" + k] - want["avg_" + k]) <= max(PSNR_TOL if k == "psnr" else DEPTH_TOL * abs(want["avg_" + k]), 0)
    assert "ms_ssim" not in result and "avg_ms_ssim" not in result
    # the files: the three score lists and the validity array; no ssim.txt without ms_ssim, and neither lpips.txt nor summary.txt at all
    assert sorted(n for n in os.listdir(eval_dir) if os.path.isfile(os.path.join(eval_dir, n))) == ["l1.txt", "psnr.txt", "rmse.txt", "valid_nvs_frames.npy"]
    for k, name in (("psnr", "psnr.txt"), ("depth_rmse", "rmse.txt"), ("depth_l1", "l1.txt")):
        assert np.array_equal(np.loadtxt(os.path.join(eval_dir, name)), result[k]), k
    saved = np.load(os.path.join(eval_dir, "valid_nvs_frames.npy"))
    assert saved.dtype == np.bool_ and saved.tolist() == [True, True, False, True]
    # the pictures, numbered by test view, under the reference's names
    names = dict(im="rendered_rgb/render_%04d.png", depth="rendered_depth/render_%04d.png", gt_im="rgb/gt_%04d.png", gt_depth="depth/gt_%04d.png")
    assert sorted(os.listdir(os.path.join(eval_dir, "rendered_rgb"))) == ["render_%04d.png" % t for t in range(4)]
    assert sum(len(os.listdir(os.path.join(eval_dir, d))) for d in ("rendered_rgb", "rendered_depth", "rgb", "depth")) == 16
    for t in (0, 2):
        im, depth, _opac, gt_im, gt_depth = (torch.tensor(a, device="cuda") for a in renders[t])
        pictures = export.export_frame(im=im, gt_im=gt_im, depth=depth, gt_depth=gt_depth)
        for key, pattern in names.items():
            with Image.open(os.path.join(eval_dir, pattern % t)) as png:
                assert png.mode == "RGB" and np.array_equal(np.asarray(png), pictures[key].cpu().numpy()), (key, t)


def test_evaluate_novel_views_eval_every_the_silhouette_branch_and_no_valid_view(nvs, tmp_path):
    from hsr_utils import evaluate
    params, cam, frames, renders = nvs
    # eval_every = 2 scores test views 0, 1 and 3; mapping_iters == 0 without new Gaussians brings the silhouette mask into the scores
    result = evaluate.evaluate_novel_views(params, frames, cam, eval_every=2, sil_thres=SIL, mapping_iters=0, add_new_gaussians=False, ms_ssim=False)
    assert result["frame_ids"] == [0, 1, 3] and result["valid_nvs_frames"].tolist() == [True, True, True]
    want = R.nvs_loop([renders[t] for t in (0, 1, 3)], SIL, 0, False)
    _check_scores(result, want, slice(None))
    assert result["avg_psnr"] == float(result["psnr"].mean()) and not os.listdir(str(tmp_path))      # nothing is written without a directory
    # a threshold no opacity passes: every valid-depth pixel is a hole, no view is valid, the averages are NaN and nothing is raised
    none = evaluate.evaluate_novel_views(params, frames, cam, str(tmp_path / "none"), sil_thres=2.0, mapping_iters=30, add_new_gaussians=True, ms_ssim=False)
    assert none["valid_nvs_frames"].tolist() == [False] * 4 and none["holes"].tolist() == none["valid_depth"].tolist()
    assert all(np.isnan(none["avg_" + k]) for k in ("psnr", "depth_l1", "depth_rmse")) and np.isfinite(none["psnr"]).all()
    assert not np.load(str(tmp_path / "none" / "valid_nvs_frames.npy")).any()


def test_evaluate_novel_views_with_ms_ssim(tmp_path):
    """MS-SSIM needs a side above 160: one view of a 176x168 map, scored with it and written as ssim.txt"""
    import hsr_utils
    from hsr_utils import evaluate, make_scene, setup_camera
    from hsr_utils.camera import replica_intrinsics
    W, H, P = 176, 168, 6000
    kmat = replica_intrinsics(W, H)
    cam = setup_camera(W, H, kmat, np.eye(4), device="cuda")
    sc = make_scene(P, W, H, 0, kmat, seed=5, kind="slam", scale_mult=2.0)
    params = {"means3D": sc["means3D"], "rgb_colors": sc["colors_precomp"], "unnorm_rotations": sc["rotations"],
              "logit_opacities": torch.logit(sc["opacities"].clamp(0.01, 0.99)), "log_scales": sc["scales"][:, :1].log()}
    params = {k: v.cuda().contiguous() for k, v in params.items()}
    w2c = VIEWS[0]
    _rv, im, _radius, _sem, depth, opac = hsr_utils.render_view(params, w2c, cam, False)
    frame = {"im": (im * 0.9).contiguous(), "depth": depth.clone(), "gt_w2c": w2c}
    result = evaluate.evaluate_novel_views(params, [frame, frame], cam, str(tmp_path), sil_thres=SIL, mapping_iters=30, add_new_gaussians=True)
    want = evaluate.ms_ssim(im, frame["im"], frame["depth"])
    assert result["ms_ssim"].shape == (1,) and result["ms_ssim"][0] == float(want) and 0 < result["ms_ssim"][0] < 1
    assert np.loadtxt(str(tmp_path / "ssim.txt")).reshape(-1)[0] == result["ms_ssim"][0]
    assert result["avg_ms_ssim"] == result["ms_ssim"][0] if result["valid_nvs_frames"][0] else np.isnan(result["avg_ms_ssim"])
