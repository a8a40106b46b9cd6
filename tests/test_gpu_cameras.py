"""-m gpu: the rasterizer under general cameras.

Every other parity test sees the world through the identity or through scenes.tilted_w2c, a turn about the y axis, under which
vm[1], vm[4], vm[6], vm[9] of the column-major viewmatrix are 0, vm[5] is 1 and projmatrix [1], [4], [7], [9] are 0: hsr_preprocess.hip
builds tvy, hy and the Wm rows of computeCov2D from those entries, hsr_backward_pre.hip its ty, Wm, the gmx / gmy / gmz chain and the
proj[..] * m_w - proj[..] * mul terms — an index or transposition error there multiplies a zero or swaps two zeros, and the y row
vm[1] x + vm[5] y + vm[9] z + vm[13] is y + t however it is associated.  Here the same comparisons run under the four cameras of
scenes.CAMERAS (tests/test_oracle_cameras.py pins the oracle under them against float64).

All comparisons go through test_gpu_parity._compare unchanged: integers and the fp32 state behind them bit for bit, the n_contrib /
median_pos budgets, floats strictly first, then the oracle's tie bound with its caps, then the truth tier."""
import ctypes as C

import numpy as np
import pytest
import torch

import scenes
import test_gpu_truth
from harness import truth_report
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

CAMS = list(scenes.CAMERAS)

# The smallest shapes at which the suite reaches every forward and backward instantiation family (test_gpu_parity.CASES), seed 11
#           W    H    P     K   kind     scale_mult semantic behind
GRID = {
    "k26":     (160, 96, 3000, 26, "aniso", 2.0,  True,  0.0),
    "k16slam": (128, 80, 2000, 16, "slam",  3.0,  True,  0.0),
    "k5":      (100, 70, 1500, 5,  "aniso", 2.5,  True,  0.0),
    "k74":     (96,  64, 1200, 74, "aniso", 2.0,  True,  0.0),
    "k33":     (96,  64, 1200, 33, "aniso", 2.0,  True,  0.0),
    "plain":   (144, 96, 2500, 0,  "aniso", 2.0,  False, 0.0),
    "behind":  (96,  64, 1500, 26, "aniso", 2.0,  True,  0.4),
    "huge":    (96,  64, 300,  26, "aniso", 40.0, True,  0.0),
}


def grid_scene(name, camera):
    """(cam, sc, up, semantic, variant, extra) of one cell of the grid"""
    W, H, P, K, kind, sm, semantic, behind = GRID[name]
    cam, sc, up = scenes.build(W, H, P, K, seed=11, kind=kind, scale_mult=sm, behind_frac=behind, w2c=scenes.CAMERAS[camera])
    return cam, sc, up, semantic, "sr", None


@pytest.mark.parametrize("name", list(GRID))
@pytest.mark.parametrize("camera", CAMS)
def test_parity_under_a_general_camera(camera, name):
    _compare(*grid_scene(name, camera))


VARIANTS = ("cov", "sh3", "mod1.7", "off_centre")


def variant_scene(variant, camera):
    """the input variants of the parity suite with the camera in place of its y-turn: cov3D_precomp (test_parity's plain_cov3d), SH of
    degree 3 (test_parity_sh), scale_modifier 1.7 (test_scale_modifier_other_than_one) and the off-centre intrinsics of
    test_gpu_fuzz.build_v2 (fx != fy, principal point off the middle)"""
    w2c = scenes.CAMERAS[camera]
    if variant == "cov":
        cam, sc, up = scenes.build(96, 80, 1500, 0, seed=11, kind="aniso", scale_mult=2.0, w2c=w2c)
        return cam, sc, up, False, "cov", {"cov3D_precomp": scenes.cov3d_from_scene(sc)}
    if variant == "sh3":
        cam, sc, up = scenes.build(96, 64, 1000, 16, seed=5, kind="aniso", scale_mult=2.0, w2c=w2c)
        cam["sh_degree"] = 3
        return cam, sc, up, True, "sr", {"shs": scenes.random_sh(1000, 16)}
    if variant == "mod1.7":
        cam, sc, up = scenes.build(150, 90, 2000, 11, seed=31, kind="aniso", scale_mult=2.0, w2c=w2c)
        return dict(cam, scale_modifier=1.7), sc, up, True, "sr", None
    assert variant == "off_centre"
    from hsr_utils.camera import setup_camera_tensors
    from hsr_utils.synthetic import make_scene, make_upstream_grads
    W, H, P, K = 160, 120, 2500, 16
    k = np.array([[0.97 * W, 0.0, 0.41 * W], [0.0, 1.07 * W, 0.57 * H], [0.0, 0.0, 1.0]])
    cam = setup_camera_tensors(W, H, k, w2c)
    assert cam["tanfovx"] / cam["tanfovy"] != W / H
    sc = make_scene(P, W, H, K, k, seed=12, kind="aniso", scale_mult=2.0, w2c=w2c)
    up = {n: v * float(W * H) for n, v in make_upstream_grads(W, H, K, seed=2).items()}
    return cam, sc, up, True, "sr", None


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("camera", ["skew23", "skew140"])
def test_input_variants_under_a_skew_camera(camera, variant):
    _compare(*variant_scene(variant, camera))


def mid_size_scene():
    """config3 of the parity suite (ScanNet 640x480, K = 16, 60 000 Gaussians) with a real camera"""
    cam, sc, up = scenes.build(640, 480, 60000, 16, seed=11, kind="slam", scale_mult=1.0, w2c=scenes.CAMERAS["skew23"])
    return cam, sc, up, True, "sr", None


def test_mid_size_frame_under_a_skew_camera():
    _compare(*mid_size_scene())


# (W, H, P, K, kind, scale_mult, seed) of test_gpu_truth's equidistance cases, each under a camera
TRUTH = [((136, 141, 2500, 26, "aniso", 3.0, 34), "skew140"), ((136, 141, 2500, 8, "aniso", 3.0, 455), "roll90")]


@pytest.mark.parametrize("cfg,camera", TRUTH, ids=["k26_skew140", "k8_roll90"])
def test_hip_and_oracle_are_equidistant_from_the_truth_under_a_general_camera(cfg, camera):
    W, H, P, K, kind, sm, seed = cfg
    cam, sc, up = scenes.build(W, H, P, K, seed=seed, kind=kind, scale_mult=sm, w2c=scenes.CAMERAS[camera])
    name = "%dx%d_P%d_K%d_%s_x%g_s%d" % cfg + "_" + camera
    test_gpu_truth._check(name, truth_report(cam, sc, up, semantic=True, atomics_seeds=test_gpu_truth.SEEDS))


@pytest.mark.parametrize("camera", CAMS)
def test_mark_visible_under_a_general_camera(camera):
    """markVisible reads the z row alone: vm[2], vm[6], vm[10], vm[14]; vm[6] is 0 under a y-turn"""
    from diff_gaussian_rasterization import GaussianRasterizer
    from harness import _cam_to
    import oracle_lib as O
    cam, sc, up = scenes.build(64, 48, 3000, 0, behind_frac=0.5, w2c=scenes.CAMERAS[camera])
    dev = torch.device("cuda:0")
    vis = GaussianRasterizer(_cam_to(cam, dev)).markVisible(sc["means3D"].to(dev)).cpu().numpy()
    P = sc["means3D"].shape[0]
    exp = np.zeros(P, np.uint8)
    m = np.ascontiguousarray(sc["means3D"].numpy()); v = np.ascontiguousarray(cam["viewmatrix"].numpy()); p = np.ascontiguousarray(cam["projmatrix"].numpy())
    O.lib().hsro_mark_visible(C.c_int(P), m.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p),
                              exp.ctypes.data_as(C.c_void_p))
    assert np.array_equal(vis, exp.astype(bool))
    assert 0 < vis.sum() < P
    # and against float64: the depth test itself, away from its threshold
    z = np.concatenate([sc["means3D"].numpy().astype(np.float64), np.ones((P, 1))], 1) @ scenes.CAMERAS[camera][2]
    sure = np.abs(z - 0.2) > 1e-5
    assert np.array_equal(vis[sure], z[sure] > 0.2) and sure.sum() > P - 5


def teardown_module(module):
    test_gpu_truth.teardown_module(module)      # this module's truth cases go into the same report file as test_gpu_truth's
