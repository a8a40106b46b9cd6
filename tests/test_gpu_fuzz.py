"""Seeded random configurations through the whole rasterizer path against the oracle: ragged image sizes, any K, tiny and
huge splats, culled points, white / coloured backgrounds.  Same checks as test_gpu_parity._compare (integers bit-exact, floats
1e-4).  Sizes are small so that the oracle finishes in well under a second per case."""
import os
import zlib

import numpy as np
import pytest

import scenes
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu


def _cases(n=28, seed=2024):
    g = np.random.default_rng(seed)
    out = []
    for i in range(n):
        W, H = int(g.integers(17, 200)), int(g.integers(17, 150))
        P = int(g.choice([1, 7, 63, 300, 1200, 2500]))
        semantic = bool(g.random() < 0.8)
        K = int(g.choice([0, 1, 3, 11, 16, 26, 27, 28, 31, 40, 52, 53, 74, 90])) if semantic else 0
        kind = str(g.choice(["slam", "aniso"]))
        sm = float(g.choice([0.3, 1.0, 3.0, 12.0, 60.0]))
        bg = tuple(float(x) for x in g.choice([0.0, 1.0, 0.3], size=3))
        behind = float(g.choice([0.0, 0.0, 0.3]))
        out.append(("%02d_%dx%d_P%d_K%d_%s_x%g" % (i, W, H, P, K, kind, sm), (W, H, P, K, kind, sm, semantic, "sr", bg, behind)))
    return out


# HSR_FUZZ_CASES / HSR_FUZZ_SEED: a longer or different run of the same generator (e.g. after a kernel change: 300 cases, another seed)
CASES = _cases(int(os.environ.get("HSR_FUZZ_CASES", "28")), int(os.environ.get("HSR_FUZZ_SEED", "2024")))


@pytest.mark.parametrize("name,cfg", CASES, ids=[c[0] for c in CASES])
def test_random_configuration(name, cfg):
    W, H, P, K, kind, sm, semantic, variant, bg, behind = cfg
    cam, sc, up = scenes.build(W, H, P, K, seed=zlib.crc32(name.encode()) % 1000, kind=kind, scale_mult=sm, bg=bg, behind_frac=behind)
    _compare(cam, sc, up, semantic, variant, None)


# Round 4: the generator above only ever draws scales + rotations with precomputed colours at scale_modifier 1
# through centred intrinsics.  A second generator — separate, so that the named cases of the first keep their seeds — also draws the
# input variant (cov3D_precomp instead of scales / rotations), the colour source (SH of degree 0..3 instead of colors_precomp), the
# scale modifier and ScanNet-like intrinsics (fx != fy, principal point off the centre).
def _cases_v2(n=24, seed=4104):
    g = np.random.default_rng(seed)
    out = []
    for i in range(n):
        W, H = int(g.integers(17, 200)), int(g.integers(17, 150))
        P = int(g.choice([7, 63, 300, 1200, 2500]))
        semantic = bool(g.random() < 0.8)
        K = int(g.choice([0, 1, 3, 11, 16, 26, 27, 28, 31, 40, 53, 74])) if semantic else 0
        kind = str(g.choice(["slam", "aniso"]))
        sm = float(g.choice([0.3, 1.0, 3.0, 12.0]))
        bg = tuple(float(x) for x in g.choice([0.0, 1.0, 0.3], size=3))
        behind = float(g.choice([0.0, 0.0, 0.3]))
        variant = str(g.choice(["sr", "cov"]))
        sh_deg = int(g.choice([-1, -1, 0, 1, 2, 3]))        # -1: colors_precomp
        mod = float(g.choice([0.6, 1.0, 1.7]))
        off_centre = bool(g.random() < 0.5)
        name = "v2_%02d_%dx%d_P%d_K%d_%s_x%g_%s_%s_mod%g_%s" % (i, W, H, P, K, kind, sm, variant, "sh%d" % sh_deg if sh_deg >= 0 else "rgb", mod,
                                                           "offc" if off_centre else "ctr")
        out.append((name, (W, H, P, K, kind, sm, semantic, variant, bg, behind, sh_deg, mod, off_centre)))
    return out


CASES_V2 = _cases_v2(int(os.environ.get("HSR_FUZZ_CASES_V2", "24")), int(os.environ.get("HSR_FUZZ_SEED_V2", "4104")))


def build_v2(name, cfg):
    import torch
    from hsr_utils.camera import setup_camera_tensors
    from hsr_utils.synthetic import make_scene, make_upstream_grads
    W, H, P, K, kind, sm, semantic, variant, bg, behind, sh_deg, mod, off_centre = cfg
    seed = zlib.crc32(name.encode()) % 1000
    if off_centre:
        k = np.array([[0.97 * W, 0.0, 0.41 * W], [0.0, 1.07 * W, 0.57 * H], [0.0, 0.0, 1.0]])
        w2c = scenes.tilted_w2c(0.15, (0.05, 0.1, 0.1))
        cam = setup_camera_tensors(W, H, k, w2c)
        cam["bg"] = torch.tensor(bg, dtype=torch.float32)
        sc = make_scene(P, W, H, K, k, seed=seed, kind=kind, scale_mult=sm, w2c=w2c, behind_frac=behind)
        up = {n: v * float(W * H) for n, v in make_upstream_grads(W, H, K, seed=1).items()}
    else:
        cam, sc, up = scenes.build(W, H, P, K, seed=seed, kind=kind, scale_mult=sm, bg=bg, behind_frac=behind)
    cam = dict(cam, scale_modifier=float(mod))
    extra = {}
    if variant == "cov":
        extra["cov3D_precomp"] = scenes.cov3d_from_scene(sc, mod)     # what the scale modifier would have made of the scales
    if sh_deg >= 0:
        cam["sh_degree"] = sh_deg
        extra["shs"] = scenes.random_sh(P, 16, seed=seed + 1)
    return cam, sc, up, semantic, variant, (extra or None)


@pytest.mark.parametrize("name,cfg", CASES_V2, ids=[c[0] for c in CASES_V2])
def test_random_configuration_variants(name, cfg):
    cam, sc, up, semantic, variant, extra = build_v2(name, cfg)
    _compare(cam, sc, up, semantic, variant, extra)


# Both generators above look through scenes.tilted_w2c, a turn about the y axis, under which the view matrix's vm[1], vm[4], vm[6], vm[9]
# are 0 and vm[5] is 1 (tests/test_gpu_cameras.py).  A third generator — separate again, so that the named cases of the first two keep their
# seeds — draws what _cases draws, plus a camera: a rotation about a random axis (normalised N(0, 1)^3) by U(0, 80) degrees and a
# translation from U(-0.5, 0.5)^3.
def _cases_v3(n=16, seed=7313):
    g = np.random.default_rng(seed)
    out = []
    for i in range(n):
        W, H = int(g.integers(17, 200)), int(g.integers(17, 150))
        P = int(g.choice([1, 7, 63, 300, 1200, 2500]))
        semantic = bool(g.random() < 0.8)
        K = int(g.choice([0, 1, 3, 11, 16, 26, 27, 28, 31, 40, 52, 53, 74, 90])) if semantic else 0
        kind = str(g.choice(["slam", "aniso"]))
        sm = float(g.choice([0.3, 1.0, 3.0, 12.0, 60.0]))
        bg = tuple(float(x) for x in g.choice([0.0, 1.0, 0.3], size=3))
        behind = float(g.choice([0.0, 0.0, 0.3]))
        axis = tuple(float(x) for x in g.standard_normal(3))
        angle = float(g.uniform(0.0, 80.0))
        t = tuple(float(x) for x in g.uniform(-0.5, 0.5, 3))
        out.append(("v3_%02d_%dx%d_P%d_K%d_%s_x%g_turn%.0f" % (i, W, H, P, K, kind, sm, angle),
                    (W, H, P, K, kind, sm, semantic, "sr", bg, behind, axis, angle, t)))
    return out


CASES_V3 = _cases_v3(int(os.environ.get("HSR_FUZZ_CASES_V3", "16")), int(os.environ.get("HSR_FUZZ_SEED_V3", "7313")))


def build_v3(name, cfg):
    W, H, P, K, kind, sm, semantic, variant, bg, behind, axis, angle, t = cfg
    cam, sc, up = scenes.build(W, H, P, K, seed=zlib.crc32(name.encode()) % 1000, kind=kind, scale_mult=sm, bg=bg, behind_frac=behind,
                               w2c=scenes.rodrigues_w2c(axis, angle, t))
    return cam, sc, up, semantic, variant, None


@pytest.mark.parametrize("name,cfg", CASES_V3, ids=[c[0] for c in CASES_V3])
def test_random_configuration_under_a_random_camera(name, cfg):
    _compare(*build_v3(name, cfg))


# the legacy accumulation mode (no scratch: atomics straight into the reference's six arrays) runs the all-VALU quadrant-list backward
# (hsr_render_bwd.hip) since round 3: every third case of the default list through it
@pytest.mark.parametrize("name,cfg", CASES[::3], ids=[c[0] for c in CASES[::3]])
def test_random_configuration_legacy_accumulation(name, cfg):
    from diff_gaussian_rasterization import _C
    W, H, P, K, kind, sm, semantic, variant, bg, behind = cfg
    cam, sc, up = scenes.build(W, H, P, K, seed=zlib.crc32(name.encode()) % 1000, kind=kind, scale_mult=sm, bg=bg, behind_frac=behind)
    _C.set_backward_mode("legacy")
    try:
        _compare(cam, sc, up, semantic, variant, None)
    finally:
        _C.set_backward_mode("packed")


# cases of the 300-case run with seed 77 that found a bug: wide-tree forward kernels left the feature row of batch slot 0 unstaged when
# no sub-block of the tile visits that splat, and a 16-lane group with an EMPTY list reads slot 0 with weight 0 — NaN * 0 when the LDS
# still held the per-tile sort's ~0 padding
_REGRESSIONS = ("108_118x88_P300_K74_aniso_x0.3", "113_195x148_P300_K31_aniso_x1", "126_128x42_P63_K74_aniso_x1",
                "167_80x101_P300_K74_aniso_x0.3", "248_139x123_P63_K27_slam_x0.3")


@pytest.mark.parametrize("name", _REGRESSIONS)
def test_regressions_found_by_longer_fuzz_runs(name):
    cfg = dict(_cases(300, 77))[name]
    W, H, P, K, kind, sm, semantic, variant, bg, behind = cfg
    cam, sc, up = scenes.build(W, H, P, K, seed=zlib.crc32(name.encode()) % 1000, kind=kind, scale_mult=sm, bg=bg, behind_frac=behind)
    _compare(cam, sc, up, semantic, variant, None)


def test_threshold_ties_are_rare_and_bounded():
    """The blend accepts a splat iff alpha = min(0.99, o * exp(power)) >= 1/255 (reference forward.cu:492-496).  A splat whose alpha
    lands within an ulp of 1/255 can be accepted by one exp implementation and rejected by another (v_exp_f32 here, glibc in the
    oracle, CUDA's expf in the reference): the pixel then differs by that splat's whole contribution, at most (1/255) * T * |c|.
    Big anisotropic splats make such ties likelier; this pins the effect on two scenes found by a seed scan (tools/scan_seeds.py):
    a handful of pixels, each within one threshold contribution, everything else within the 1e-4 bar."""
    from harness import run_gpu, run_oracle
    W, H, P, K = 136, 141, 2500, 26
    for seed in (34, 40):
        cam, sc, up = scenes.build(W, H, P, K, seed=seed, kind="aniso", scale_mult=3.0, bg=(0, 0, 0), behind_frac=0.0)
        og, gg, sg = run_gpu(cam, sc, up, semantic=True, variant="sr")
        oo, go, so = run_oracle(cam, sc, up, semantic=True, variant="sr")
        assert np.array_equal(sg["keys"], so.field("keys")) and np.array_equal(og["radii"], oo["radii"])
        err = np.abs(np.asarray(og["color"], np.float64) - np.asarray(oo["color"], np.float64).reshape(3, H, W)).max(axis=0)
        bad = err > 1e-4
        assert int(bad.sum()) <= 8, int(bad.sum())              # whether the two exps disagree here or not: at most a handful of pixels
        assert float(err.max()) <= 1.05 / 255.0                 # one splat at the 1/255 threshold, colour <= 1
        # and every pixel that does differ is one the oracle flagged, within the bound it computed for it
        bound = so.img_bound("color").reshape(H, W).astype(np.float64)
        assert (err <= 1e-4 + 1.1 * bound).all(), float((err - 1.1 * bound).max())
