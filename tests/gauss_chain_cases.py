"""Scenes for the per-Gaussian chain of the rasterizer (hsr_backward_pre.hip, and the float state hsr_preprocess.hip writes for it), with a
Gaussian at every branch of that code.  tests/test_gauss_chain_cpu.py holds every directed Gaussian to the regime it is named for on the
oracle's forward state; tests/test_gpu_gauss_chain.py runs every case on the device.

    CASES            name -> builder of a Case; the directed scene in seven variants, then five random scenes (two of them under general cameras)
    directed_info()  name of a directed Gaussian -> its index in the directed scene, its group and the regime it is meant for
    prefix(n)        the first n Gaussians of the directed scene

The directed scene: 64 x 48, identity w2c (the view depth is z bit for bit, t = mean), P = 600.  Directed Gaussians stand on the seams
of the kernel's blocks, waves and passes — 0, 63, 64, 127, 128, 255, 256, 257, 599 — and on every eleventh index from 270 on; Gaussians
of make_scene(kind="aniso") fill the rest.

    near        z = 0.2f (culled: tvz <= 0.2f), the float below it (culled), the float above it (kept)
    clamp       z = 1; x/z at L = 1.3f * tanfovx in fp32 (as the kernel forms it), one ulp inside, one ulp outside, 1.6 L, the negatives; the
                same for y; one outside on both axes.  Scales of 0.3-0.45, so that each still touches the screen.
    radius      scales of 1e-6: cov2D = 0.3 I, the max(0.1, mid^2 - det) floor decides, radius 3.  Centres found by search, so that
                (p - r) / 16 and ((p + r) + 16 - 1) / 16 are exact integers; centres outside the image whose rectangle is clamped to the
                first / the last tile column; a centre whose rectangle is empty (culled at a visible depth); one splat on every tile
    rot_scale   quaternions (0,0,0,0), of norm 2 and 0.5; one scale axis 0; needles of 30:1 and 300:1
    opacity     0, 1/512, 1/255 (fp32): visible, but alpha < 1/255 on every pixel — zero-filled packed rows that stay zero
    cov         (cov3D_precomp variant only) a row whose cov2D + 0.3 I is [[1, 1], [1, 1]] exactly — det == 0, culled — and one with a det of
                1e-4 (denom2inv of 9e6); both at (0, 0, 1), where T = diag(focal_x, focal_y)
    sh          (SH variants only) Gaussian 256: channel 1 far below the clamp, channel 2 equal to 0.0f after the + 0.5f (not clamped:
                r < 0 is false), in every degree; every fifth Gaussian has channel 1 pushed below the clamp

The searches run on the CPU oracle itself (its forward state), so what they find is right by the rule the device is held to."""
import functools
from collections import namedtuple

import numpy as np
import torch

import oracle_lib as O
import scenes

Case = namedtuple("Case", "cam sc up variant extra")      # variant / extra as harness.variant_kwargs takes them

W, H, P, K = 64, 48, 600, 26
SEAMS = (0, 63, 64, 127, 128, 255, 256, 257, 599)
F32 = np.float32
SH_C0 = F32(0.28209479177387814)


def _ulps(x, k):
    """the fp32 k floats above (k > 0) or below x, for x != 0: arrays of k broadcast"""
    x = F32(x)
    i = np.asarray(x).view(np.int32).astype(np.int64)
    return (i + (np.asarray(k, np.int64) if x > 0 else -np.asarray(k, np.int64))).astype(np.int32).view(np.float32)


def _base():
    return scenes.build(W, H, P, K, seed=41, kind="aniso", scale_mult=2.0, tilt=False)


def limits(cam):
    """(limx, limy): 1.3f * tan_fov as the kernels form them, in fp32"""
    return F32(1.3) * F32(cam["tanfovx"]), F32(1.3) * F32(cam["tanfovy"])


@functools.lru_cache(maxsize=None)
def _centre_for_pixel(axis, target, exact=True):
    """the camera-space x (axis 0) or y (axis 1) at z = 1 whose projected pixel coordinate is `target` exactly, by the oracle's forward
    (exact=False: to within rounding — for centres whose splat is culled, which leave no state to search on)"""
    cam, _, _ = _base()

    def pix(v):
        n = v.shape[0]
        m = np.zeros((n, 3), np.float32)
        m[:, axis], m[:, 2] = v, 1.0
        _, st = O.forward(cam, m, np.full((n, 1), 0.5, np.float32), colors_precomp=np.zeros((n, 3), np.float32),
                          scales=np.full((n, 3), 1e-6, np.float32), rotations=np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1)))
        out = st.field("means2D")[:, axis].copy()      # a culled candidate's stays 0
        st.free()
        return out
    a, b = pix(np.array([0.0, 0.25], np.float32))
    x0 = F32((target - a) / (b - a) * 0.25)
    if not exact:
        return float(x0)
    cand = _ulps(x0, np.arange(-512, 513))
    hit = np.flatnonzero(pix(cand) == F32(target))
    assert hit.size, "no fp32 centre projects to pixel %r on axis %d" % (target, axis)
    return float(cand[hit[np.abs(hit - 512).argmin()]])


@functools.lru_cache(maxsize=None)
def _singular_cov():
    """(V00, V01, V11) of a cov3D row at mean (0, 0, 1) whose cov2D + 0.3 I is [[1, 1], [1, 1]] bit for bit: det == 0.0f"""
    cam, _, _ = _base()
    fx, fy = F32(W) / (F32(2.0) * F32(cam["tanfovx"])), F32(H) / (F32(2.0) * F32(cam["tanfovy"]))
    out = []
    for ta, tb in ((fx, fx), (fx, fy), (fy, fy)):
        cand = _ulps(F32(0.7 if ta == tb else 1.0) / (ta * tb), np.arange(-4096, 4097))
        # cov2D[col c][row r] = (t_r * V_rc) * t_c, and the kernels read the off-diagonal entry at column 0, row 1
        c = (F32(tb) * cand) * F32(ta) + (F32(0.3) if ta == tb else F32(0.0))
        hit = np.flatnonzero(c == F32(1.0))
        assert hit.size
        out.append(float(cand[hit[np.abs(hit - 4096).argmin()]]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _sh0_for_zero():
    """the degree-0 coefficient c with fl(SH_C0 * c) + 0.5f == 0.0f"""
    cand = _ulps(F32(-0.5) / SH_C0, np.arange(-64, 65))
    hit = np.flatnonzero(SH_C0 * cand + F32(0.5) == F32(0.0))
    assert hit.size
    return float(cand[hit[np.abs(hit - 64).argmin()]])


def _quat(seed, norm):
    q = np.random.default_rng(seed).standard_normal(4)
    return tuple(float(v) for v in q / np.linalg.norm(q) * norm)


IDENT = (1.0, 0.0, 0.0, 0.0)
TILTED = _quat(1, 1.0)


def _directed(cam):
    """[(name, group, mean, scales, quaternion, opacity, expectations)], in the order in which they take SEAMS and then 270, 281, ...
    expectations: visible; radius / tiles where the table fixes them; clamp = (side of x, side of y) out of "in" / "on" / "out"; floor"""
    limx, limy = limits(cam)
    near = F32(0.2)
    big, tiny = (0.45, 0.3, 0.35), (1e-6, 1e-6, 1e-6)
    cx = lambda t: _centre_for_pixel(0, t)
    cy = lambda t: _centre_for_pixel(1, t)
    x_in, y_in = 0.05, 0.1
    g = []
    add = lambda name, group, mean, s, q=IDENT, o=0.6, **exp: g.append((name, group, tuple(float(v) for v in mean), s, q, o, exp))
    # ---- the seams ----
    add("clamp_x_out", "clamp", (_ulps(limx, 1), y_in, 1.0), big, TILTED, visible=True, clamp=("out", "in"))              # 0
    add("near_below", "near", (0.0, 0.0, _ulps(near, -1)), (0.005,) * 3, visible=False)                                   # 63
    add("near_above", "near", (0.0, 0.0, _ulps(near, 1)), (0.005,) * 3, visible=True)                                     # 64
    add("cov_det0", "cov", (0.0, 0.0, 1.0), (0.05, 0.03, 0.04), TILTED, visible=True)                                     # 127
    add("cov_det1e-4", "cov", (0.0, 0.0, 1.0), (0.04, 0.05, 0.03), TILTED, visible=True)                                  # 128
    add("rect_empty", "radius", (_centre_for_pixel(0, -10.0, exact=False), cy(20.5), 1.0), tiny, visible=False)                                          # 255
    add("every_tile", "radius", (0.01, -0.02, 1.0), (2.0, 1.2, 1.6), TILTED, visible=True, tiles=12, floor=False)         # 256
    add("needle_300", "rot_scale", (0.3, 0.1, 2.0), (0.6, 0.002, 0.002), _quat(2, 1.0), visible=True)                     # 257
    add("quat_zero", "rot_scale", (-0.2, 0.1, 1.5), (0.08, 0.05, 0.1), (0.0, 0.0, 0.0, 0.0), visible=True)               # 599
    # ---- 270, 281, ... ----
    add("near_at", "near", (0.0, 0.0, near), (0.005,) * 3, visible=False)
    for name, x, side in (("on", limx, "on"), ("in", _ulps(limx, -1), "in"), ("far", F32(1.6) * limx, "out")):
        add("clamp_x_" + name, "clamp", (x, y_in, 1.0), big, TILTED, visible=True, clamp=(side, "in"))
    for name, x, side in (("on", limx, "on"), ("in", _ulps(limx, -1), "in"), ("out", _ulps(limx, 1), "out"), ("far", F32(1.6) * limx, "out")):
        add("clamp_-x_" + name, "clamp", (-x, y_in, 1.0), big, TILTED, visible=True, clamp=(side, "in"))
    for sgn, tag in ((1.0, "y"), (-1.0, "-y")):
        for name, y, side in (("on", limy, "on"), ("in", _ulps(limy, -1), "in"), ("out", _ulps(limy, 1), "out"), ("far", F32(1.6) * limy, "out")):
            add("clamp_%s_%s" % (tag, name), "clamp", (x_in, sgn * y, 1.0), big, TILTED, visible=True, clamp=("in", side))
    add("clamp_xy_out", "clamp", (_ulps(limx, 1), -_ulps(limy, 1), 1.0), big, TILTED, visible=True, clamp=("out", "out"))
    # radius 3: (19 - 3) / 16 = 1 and (19 + 3 + 15) / 16 = 2.3: one tile, where a centre one float lower would take two columns and rows
    add("rect_min_edge", "radius", (cx(19.0), cy(19.0), 1.0), tiny, visible=True, radius=3, tiles=1, floor=True)
    # (30 + 3 + 16 - 1) / 16 = 3 and (14 + 3 + 16 - 1) / 16 = 2: columns 1-2 and rows 0-1
    add("rect_max_edge", "radius", (cx(30.0), cy(14.0), 1.0), tiny, visible=True, radius=3, tiles=4, floor=True)
    add("rect_first_column", "radius", (cx(-2.0), cy(20.5), 1.0), tiny, visible=True, radius=3, tiles=1, floor=True)        # (-2 + 18) / 16 = 1
    add("rect_last_column", "radius", (cx(65.5), cy(20.5), 1.0), tiny, visible=True, radius=3, tiles=1, floor=True)         # max clamped to 4
    add("quat_norm_2", "rot_scale", (0.2, -0.1, 1.5), (0.05, 0.1, 0.03), _quat(3, 2.0), visible=True)
    add("quat_norm_half", "rot_scale", (-0.1, -0.15, 1.5), (0.05, 0.1, 0.03), _quat(4, 0.5), visible=True)
    add("scale_axis_0", "rot_scale", (0.1, 0.2, 1.5), (0.08, 0.0, 0.05), _quat(5, 1.0), visible=True)
    add("needle_30", "rot_scale", (-0.3, -0.1, 2.0), (0.3, 0.01, 0.01), _quat(6, 1.0), visible=True)
    # centres half a pixel off the pixel grid: G < 1 everywhere, so alpha = opacity * G < 1/255 on every pixel
    for name, o, px in (("0", 0.0, 38.5), ("1_512", 1.0 / 512, 44.5), ("1_255", float(F32(1.0) / F32(255.0)), 50.5)):
        add("opacity_" + name, "opacity", (cx(px), cy(30.5), 1.0), (0.06, 0.06, 0.06), IDENT, o, visible=True)
    return g


def _indices(n):
    idx = list(SEAMS) + [270 + 11 * j for j in range(n - len(SEAMS))]
    assert len(set(idx)) == n and max(idx) <= P - 1
    return idx


@functools.lru_cache(maxsize=None)
def _directed_scene():
    cam, sc, up = _base()
    table = _directed(cam)
    sc = {n: v.clone() for n, v in sc.items()}
    info = {}
    for i, (name, group, mean, s, q, o, exp) in zip(_indices(len(table)), table):
        sc["means3D"][i] = torch.tensor(mean, dtype=torch.float64).float()
        sc["scales"][i] = torch.tensor(s, dtype=torch.float64).float()
        sc["rotations"][i] = torch.tensor(q, dtype=torch.float64).float()
        sc["opacities"][i, 0] = float(o)
        info[name] = dict(exp, index=i, group=group)
    return cam, sc, up, info


def directed_info():
    """name -> dict(index, group, visible, and radius / tiles / clamp / floor where the table fixes them)"""
    return _directed_scene()[3]


def index_of(name):
    return directed_info()[name]["index"]


SH_GAUSSIAN = 256     # "every_tile".  SH variants: channel 1 below the clamp, channel 2 at 0.0f exactly, in every degree


def directed_cov3d(sc, mod=1.0):
    cov = scenes.cov3d_from_scene(sc, mod)
    v00, v01, v11 = _singular_cov()
    cov[index_of("cov_det0")] = torch.tensor([v00, v01, 0.0, v11, 0.0, 1e-4])
    # cov2D + 0.3 I = [[1, c], [c, 1]] with c^2 = 1 - 1e-4
    cov[index_of("cov_det1e-4")] = torch.tensor([v00, v01 * float(np.sqrt(1.0 - 1e-4)), 0.0, v11, 0.0, 1e-4])
    return cov


def directed_sh(n=P):
    sh = scenes.random_sh(P, 16, seed=23)
    sh[2::5, 0, 1] = -2.5                                   # 0.28 * -2.5 + 0.5 < 0 before the higher degrees: mostly clamped
    sh[SH_GAUSSIAN, :, 1:] = 0.0
    sh[SH_GAUSSIAN, 0, 1] = -3.0                            # r = -0.35 in every degree
    sh[SH_GAUSSIAN, 0, 2] = _sh0_for_zero()                 # r = -0.5f + 0.5f (+- 0 from the higher degrees) = 0.0f
    return sh[:n].contiguous()


def directed(variant="sr", mod=1.0, sh_degree=None, n=P):
    """the directed scene (its first n Gaussians) as a Case"""
    cam, sc, up, _ = _directed_scene()
    cam = dict(cam, scale_modifier=float(mod))
    sc = {k: v[:n].contiguous() for k, v in sc.items()}
    extra = {}
    if variant == "cov":
        extra["cov3D_precomp"] = directed_cov3d(_directed_scene()[1], mod)[:n].contiguous()
    if sh_degree is not None:
        cam["sh_degree"] = int(sh_degree)
        extra["shs"] = directed_sh(n)
    return Case(cam, sc, up, variant, extra or None)


def prefix(n):
    return directed(n=n)


def _random(Wr, Hr, seed, scale_mult, off_centre=False, sh_degree=None, camera=None):
    """camera: a name of scenes.CAMERAS, in place of the turn about y"""
    assert camera is None or not off_centre
    if off_centre:      # the intrinsics of test_off_centre_principal_point_and_unequal_focal_lengths, at this size
        from hsr_utils.camera import setup_camera_tensors
        from hsr_utils.synthetic import make_scene, make_upstream_grads
        k = np.array([[0.97 * Wr, 0.0, 0.41 * Wr], [0.0, 1.07 * Wr, 0.57 * Hr], [0.0, 0.0, 1.0]])
        w2c = scenes.tilted_w2c(0.15, (0.05, 0.1, 0.1))
        cam = setup_camera_tensors(Wr, Hr, k, w2c)
        sc = make_scene(P, Wr, Hr, K, k, seed=seed, kind="aniso", scale_mult=scale_mult, w2c=w2c)
        up = {n: v * float(Wr * Hr) for n, v in make_upstream_grads(Wr, Hr, K, seed=1).items()}
    else:
        cam, sc, up = scenes.build(Wr, Hr, P, K, seed=seed, kind="aniso", scale_mult=scale_mult,
                                   w2c=None if camera is None else scenes.CAMERAS[camera])
    extra = None
    if sh_degree is not None:
        cam = dict(cam, sh_degree=int(sh_degree))
        extra = {"shs": scenes.random_sh(P, 16, seed=seed + 1)}
    return Case(cam, sc, up, "sr", extra)


CASES = {
    "directed": lambda: directed(),
    "directed_mod1.7": lambda: directed(mod=1.7),
    "directed_cov": lambda: directed("cov"),
    "directed_sh0": lambda: directed(sh_degree=0),
    "directed_sh1": lambda: directed(sh_degree=1),
    "directed_sh2": lambda: directed(sh_degree=2),
    "directed_sh3": lambda: directed(sh_degree=3),
    "random_64x48_x2": lambda: _random(64, 48, 51, 2.0),
    "random_100x70_x40": lambda: _random(100, 70, 52, 40.0),
    "random_100x70_off_centre_sh3": lambda: _random(100, 70, 53, 2.0, off_centre=True, sh_degree=3),
    # general cameras: every entry of the view matrix that the chain reads is live (tests/test_gpu_cameras.py)
    "random_64x48_x2_skew23": lambda: _random(64, 48, 54, 2.0, camera="skew23"),
    "random_100x70_x2_skew140_sh3": lambda: _random(100, 70, 55, 2.0, sh_degree=3, camera="skew140"),
}
