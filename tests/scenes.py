"""Seeded test scenes shared by the CPU and GPU suites (inputs only; expectations come from the oracle)."""
import math

import numpy as np
import torch

from hsr_utils.camera import replica_intrinsics, setup_camera_tensors
from hsr_utils.synthetic import make_scene, make_upstream_grads


def tilted_w2c(angle=0.2, t=(0.1, -0.05, 0.2)):
    w2c = np.eye(4)
    w2c[:3, :3] = np.array([[math.cos(angle), 0, math.sin(angle)], [0, 1, 0], [-math.sin(angle), 0, math.cos(angle)]])
    w2c[:3, 3] = t
    return w2c


def rodrigues_w2c(axis, degrees, t):
    """w2c [4,4] float64: the rotation by `degrees` about `axis` (Rodrigues' formula) and the translation t"""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = np.deg2rad(degrees)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    w2c = np.eye(4)
    w2c[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
    w2c[:3, 3] = t
    return w2c


# General cameras.  tilted_w2c is a turn about y: R01 = R10 = R12 = R21 = 0 and R11 = 1, so in the kernels' column-major viewmatrix vm[1],
# vm[4], vm[6], vm[9] are 0 and vm[5] is 1 (projmatrix [1], [4], [7], [9] are 0 too) — an index or transposition error in the y row or
# column of any projection multiplies a zero or swaps two zeros, and y = 1 * y + t however the sum is associated.  These four are the
# cameras under which no view-matrix entry the kernels read is 0 or 1 in all cases (tests/test_oracle_cameras.py holds them to that):
#   skew23    every entry non-trivial, a small angle (the matrix tests/test_gpu_view.py calls "tilted")
#   skew140   every entry large (the smallest |R entry| is 0.108), negative diagonal
#   roll90    x and y exchanged exactly: a transposed index becomes a sign or axis error
#   pitch17   the complement of the y-turn: R12 and R21 are live, the x row is trivial
CAMERAS = {
    "skew23": rodrigues_w2c((0.9, 0.2, -0.1), 23.0, (0.3, -0.2, 0.5)),
    "skew140": rodrigues_w2c((0.3, -0.8, 0.5), 140.0, (-0.4, 0.1, 0.6)),
    "roll90": rodrigues_w2c((0.0, 0.0, 1.0), 90.0, (0.1, 0.2, -0.1)),
    "pitch17": rodrigues_w2c((1.0, 0.0, 0.0), -17.0, (0.0, 0.3, 0.2)),
}


def build(W, H, P, K, seed=0, kind="aniso", scale_mult=2.0, tilt=True, bg=(0.0, 0.0, 0.0), behind_frac=0.0, grad_seed=1,
          grad_scale=None, w2c=None):
    """w2c: a camera (one of CAMERAS, or any 4x4) in place of the y-turn, for the camera tensors and for placing the scene"""
    k = replica_intrinsics(W, H)
    if w2c is not None:
        w2c, tilt = np.asarray(w2c, np.float64), True
    else:
        w2c = tilted_w2c() if tilt else np.eye(4)
    cam = setup_camera_tensors(W, H, k, w2c)
    cam["bg"] = torch.tensor(bg, dtype=torch.float32)
    sc = make_scene(P, W, H, K, k, seed=seed, kind=kind, scale_mult=scale_mult, w2c=w2c if tilt else None,
                    behind_frac=behind_frac)
    up = make_upstream_grads(W, H, K, seed=grad_seed)
    s = float(W * H) if grad_scale is None else grad_scale
    up = {n: v * s for n, v in up.items()}  # O(1) upstream grads: errors then read as relative
    return cam, sc, up


def sensor_grid_depth(xs, ys, H, step_mm, z0=2.0):
    """the depth image of sensor_grid at pixel centres (xs, ys), float32 torch ops: a ramp along x that starts z0 metres away, a step of
    half a metre below the middle row, quantised to step_mm millimetres — what a depth sensor hands over"""
    z = z0 + 0.004 * xs + 0.5 * (ys > H / 2).float()
    return (torch.round(z * 1000.0 / step_mm) * step_mm / 1000.0).float()


def sensor_grid(W, H, K, sigma_px, step_mm, opacity, stride=1, seed=0, shuffle=False, duplicate_first=0, z0=2.0):
    """A first-frame-style map: one isotropic Gaussian of sigma_px pixels on every stride-th pixel of a quantised depth image, viewed
    from the identity pose (what hsr_utils.slam.initialize_first_timestep builds from frame 0).  Fronto-parallel surfaces give many
    splats of a tile the SAME depth bits, so the order of the sorted lists among them is decided by the Gaussian index alone.
    opacity: a float for every Gaussian, or (lo, hi) for lo + (hi - lo) * rand.  shuffle: permute the Gaussians, so that the index
    order no longer follows the raster order.  duplicate_first = n: append copies of the first n Gaussians (densification over
    existing points: identical mean and depth, larger index).  z0: the near end of the depth ramp; the splats' footprints in pixels do not
    depend on it.  Returns (cam, sc, up) like build()."""
    k = replica_intrinsics(W, H)
    fx, fy, cx, cy = k[0][0], k[1][1], k[0][2], k[1][2]
    cam = setup_camera_tensors(W, H, k, np.eye(4))
    cam["bg"] = torch.zeros(3, dtype=torch.float32)
    ys, xs = torch.meshgrid(torch.arange(0, H, stride), torch.arange(0, W, stride), indexing="ij")   # row-major
    xs, ys = xs.reshape(-1).float(), ys.reshape(-1).float()
    z = sensor_grid_depth(xs, ys, H, step_mm, z0)
    means = torch.stack([((xs - cx) / fx) * z, ((ys - cy) / fy) * z, z], 1)
    P = means.shape[0]
    s = (z / (0.5 * (fx + fy))) * sigma_px
    rots = torch.zeros(P, 4)
    rots[:, 0] = 1
    g = torch.Generator(device="cpu").manual_seed(seed)
    colors = torch.rand(P, 3, generator=g)
    sems = torch.rand(P, K, generator=g)
    if isinstance(opacity, (tuple, list)):
        lo, hi = opacity
        opac = (lo + (hi - lo) * torch.rand(P, 1, generator=torch.Generator(device="cpu").manual_seed(5))).float()
    else:
        opac = torch.full((P, 1), float(opacity))
    sc = dict(means3D=means, scales=s[:, None].repeat(1, 3), rotations=rots, opacities=opac, colors_precomp=colors,
              semantics_precomp=sems)
    if shuffle:
        perm = torch.randperm(P, generator=torch.Generator(device="cpu").manual_seed(3))
        sc = {n: v[perm] for n, v in sc.items()}
    if duplicate_first:
        sc = {n: torch.cat([v, v[:duplicate_first]], 0) for n, v in sc.items()}
    sc = {n: v.float().contiguous() for n, v in sc.items()}
    up = {n: v * float(W * H) for n, v in make_upstream_grads(W, H, K, seed=1).items()}
    return cam, sc, up


# First-frame-style maps on which equal depths decide the list order (tests/test_depth_ties_cpu.py holds each to the regime it was
# chosen for; tests/test_gpu_depth_ties.py runs them on the device).  The per-tile sort's size classes (hsr_sort.hip): <= 256, 257-512
# and 513-1024 entries are sorted by two waves in registers, 1025-2048 by the whole workgroup, more by the block radix sort.
# name: (sensor_grid arguments, class of the smallest tile's entry count, class of the largest tile's, compare floats too)
UP_TO_256, TO_512, TO_1024, TO_2048, BLOCK_RADIX = (1, 256), (257, 512), (513, 1024), (1025, 2048), (2049, 1 << 30)
_FIRST = dict(W=96, H=64, K=5, sigma_px=1.0, step_mm=1.0, opacity=0.5)
_WIDE = dict(W=64, H=48, K=26, sigma_px=3.0, step_mm=50.0, opacity=0.37)
TIE_CASES = {
    "first_frame": (_FIRST, TO_512, TO_1024, True),
    "first_frame_shuffled": (dict(_FIRST, shuffle=True), TO_512, TO_1024, True),
    "wide": (_WIDE, TO_1024, TO_2048, True),
    "wide_shuffled": (dict(_WIDE, shuffle=True), TO_1024, TO_2048, True),
    # P = 3 072: two index passes before the four depth passes of the block radix sort, six in all
    "deep": (dict(W=64, H=48, K=3, sigma_px=6.0, step_mm=250.0, opacity=(0.03, 0.2)), TO_2048, BLOCK_RADIX, True),
    # P = 69 888 > 65 536: three index passes, seven in all — an odd count, so the segment is copied home at the end.  Integers only: at
    # a million list entries the fp32 oracle and its truth build already take a few alpha >= 1/255 decisions differently.
    "deep_65537": (dict(W=336, H=208, K=3, sigma_px=7.0, step_mm=250.0, opacity=0.05), TO_2048, BLOCK_RADIX, False),
    # The same with the ramp starting at 1 m, so that depths on both sides of 2.0 meet in tiles beyond 2 048 entries.  With depths of
    # 2-4 m alone the most significant depth byte is 0x40 everywhere, the seventh pass moves nothing, and the sorted pair holds the right
    # order even if the copy home is left out (found with a build that leaves it out: deep_65537 passed, this case fails).
    "deep_65537_two_exponents": (dict(W=336, H=208, K=3, sigma_px=7.0, step_mm=250.0, opacity=0.05, z0=1.0), TO_2048, BLOCK_RADIX, False),
    "small": (dict(W=48, H=32, K=5, sigma_px=1.0, step_mm=50.0, opacity=0.37, stride=2), UP_TO_256, UP_TO_256, True),
    "one_tile_256": (dict(W=16, H=16, K=3, sigma_px=1.0, step_mm=250.0, opacity=0.3), (256, 256), (256, 256), True),
    "duplicates": (dict(_FIRST, duplicate_first=1000), TO_512, TO_1024, True),
}


def tie_share(keys):
    """share of adjacent sorted entries with equal keys (same tile, same depth bits)"""
    keys = np.asarray(keys)
    return float((keys[1:] == keys[:-1]).mean()) if keys.size > 1 else 0.0


def assert_ties_in_index_order(keys, vals):
    """among equal keys the values (Gaussian indices) strictly ascend: the stable sort's rule (rasterizer_impl.cu:307-312)"""
    keys, vals = np.asarray(keys), np.asarray(vals).astype(np.int64)
    eq = keys[1:] == keys[:-1]
    bad = eq & (vals[1:] <= vals[:-1])
    assert not bad.any(), "%d of %d equal-key neighbours are not in ascending Gaussian order (first at list position %d)" % (
        int(bad.sum()), int(eq.sum()), int(np.flatnonzero(bad)[0]))


def cov3d_from_scene(sc, mod=1.0):
    """world covariance [P,6] from scales/rotations (float64 maths, rounded to fp32) for the cov3D_precomp path"""
    s = sc["scales"].double() * mod
    q = sc["rotations"].double()
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    Sig = R @ torch.diag_embed(s * s) @ R.transpose(1, 2)
    return torch.stack([Sig[:, 0, 0], Sig[:, 0, 1], Sig[:, 0, 2], Sig[:, 1, 1], Sig[:, 1, 2], Sig[:, 2, 2]], 1).float().contiguous()


def random_sh(P, M, seed=7):
    g = torch.Generator(device="cpu").manual_seed(seed)
    sh = torch.randn(P, M, 3, generator=g) * 0.3
    sh[:, 0, :] += 0.8
    return sh.float().contiguous()
