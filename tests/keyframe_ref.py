"""Torch restatement of the reference's keyframe selection (utils/keyframe_selection.py:10-96), the checker of hsr_utils/keyframes.py.
Line numbers cite utils/keyframe_selection.py.  Any device, any floating dtype: fp32 on the CPU it is the reference's own arithmetic
(the fixtures of tests/golden/keyframes pin that), float64 gives the decisions the borderline rule is measured from, and on the GPU
with loop=True it is the eager chain tools/bench_keyframes.py times.

Borderline rule (tests/golden/make_keyframe_golden.py asserts it against the reference's own fp32 values): with everything evaluated in
float64 from the inputs, a (point, keyframe) pair is borderline when |zz| <= TAU * S_z, or zz > 0 and u or v lies within
m = TAU * (|u| + |v| + W + H) * S_z / |zz| of one of its two thresholds; TAU = 64 * 2^-24 (about 16 fp32 roundings on the way to u,
scaled by the condition of the division, times a safety factor of 4) and S_z = the sum of the magnitudes of the terms of zz.  Off the
borderline every fp32 evaluation order takes the float64 decision; on it either decision is accepted, so a keyframe's count may differ
from the float64 count by at most its number b of borderline pairs.
"""
import numpy as np
import torch

EDGE = 20                      # :78
TAU = 64.0 * 2.0 ** -24


def valid_pixels(gt_depth):
    """[N,2] int64 (row, col) of the pixels with depth > 0, row-major (:56-57)."""
    return torch.stack(torch.where(gt_depth[0] > 0), dim=1)


def back_project(gt_depth, intrinsics, w2c, sampled_indices, dtype=torch.float32):
    """get_pointcloud before its removal step (:11-25): world points [n,3] of the sampled (row, col) pixels."""
    K, depth = intrinsics.to(dtype), gt_depth.to(dtype)
    cx, cy, fx, fy = K[0][2], K[1][2], K[0][0], K[1][1]
    xx = (sampled_indices[:, 1].to(dtype) - cx) / fx                                 # :17
    yy = (sampled_indices[:, 0].to(dtype) - cy) / fy                                 # :18
    z = depth[0, sampled_indices[:, 0], sampled_indices[:, 1]]                       # :19
    cam = torch.stack((xx * z, yy * z, z), dim=-1)                                   # :22
    pts4 = torch.cat([cam, torch.ones_like(cam[:, :1])], dim=1)                      # :23
    c2w = torch.inverse(w2c.to(dtype))                                               # :24
    return (c2w @ pts4.T).T[:, :3]                                                   # :25


def round_key(pts):
    """|round(pts, decimals=4)| (:28)."""
    return torch.abs(torch.round(pts, decimals=4))


def keep_by_keys(pts):
    """bool [n]: False where the point's key is (0, 0, 0) or equals another point's key (:28-34): the rows of [keys; 0] that unique()
    counts more than once."""
    A = round_key(pts)
    rows = torch.cat([A, torch.zeros((1, 3), dtype=A.dtype, device=A.device)], dim=0)
    _, inverse, counts = rows.unique(dim=0, return_inverse=True, return_counts=True)
    return (counts[inverse] == 1)[:len(A)]


def keep_by_pixels(sampled_indices, pts):
    """What keep_by_keys amounts to when no two different pixels share a key: False where the pixel was drawn more than once or the
    point's key is the origin's.  Independent of the dtype the points were computed in (the float64 runs use it)."""
    _, inverse, counts = sampled_indices.unique(dim=0, return_inverse=True, return_counts=True)
    origin = (round_key(pts.float()) == 0).all(dim=1)
    return (counts[inverse] == 1) & ~origin


def project(pts, poses, intrinsics, W, H, dtype=torch.float32):
    """u, v, zz, inside — each [n_kf, n] — of :69-81 for the stacked est_w2c `poses` [n_kf,4,4]."""
    pts, poses, K = pts.to(dtype), poses.to(dtype), intrinsics.to(dtype)
    pts4 = torch.cat([pts, torch.ones_like(pts[:, :1])], dim=1)                      # :69
    cam = (poses @ pts4.T)[:, :3, :]                                                 # :70  [n_kf,3,n]
    p2d = K @ cam                                                                    # :72
    zz = p2d[:, 2] + 1e-5                                                            # :74
    u, v = p2d[:, 0] / zz, p2d[:, 1] / zz                                            # :75-76
    inside = (u < W - EDGE) & (u > EDGE) & (v < H - EDGE) & (v > EDGE) & (zz > 0)    # :79-81
    return u, v, zz, inside


def borderline(pts64, poses, intrinsics, W, H):
    """float64 decisions and the borderline marks.  Returns (inside [n_kf,n] bool, border [n_kf,n] bool, u, v, m)."""
    dt = torch.float64
    pts64, poses, K = pts64.to(dt), poses.to(dt), intrinsics.to(dt)
    u, v, zz, inside = project(pts64, poses, K, W, H, dt)
    pts4 = torch.cat([pts64, torch.ones_like(pts64[:, :1])], dim=1)
    s_cam = (poses.abs() @ pts4.abs().T)[:, :3, :]                                   # sum of |terms| of each camera coordinate
    s_z = (K.abs() @ s_cam)[:, 2] + 1e-5
    m = TAU * (u.abs() + v.abs() + W + H) * s_z / zz.abs()
    near = ((u - (W - EDGE)).abs() <= m) | ((u - EDGE).abs() <= m) | ((v - (H - EDGE)).abs() <= m) | ((v - EDGE).abs() <= m)
    border = (zz.abs() <= TAU * s_z) | ((zz > 0) & near)
    return inside, border, u, v, m


def selection_order(counts):
    """ids with a non-zero count, by count descending, ties in list order: what the stable sorted(reverse=True) of :88-92 leaves."""
    c = np.asarray(counts, dtype=np.int64)
    return [int(i) for i in np.argsort(-c, kind="stable") if c[i] > 0]


def overlap(gt_depth, w2c, intrinsics, poses, pixels=1600, dtype=torch.float32):
    """The selection up to the counts, vectorised over the keyframes; draws the ranks as :58 does (CPU default generator).  Returns a
    dict: pixels [n,2] int64, keep [n] bool, pts [m,3] (survivors), counts int64 [n_kf] (numpy), inside [n_kf,m] bool."""
    H, W = gt_depth.shape[1], gt_depth.shape[2]
    valid = valid_pixels(gt_depth)
    indices = torch.randint(valid.shape[0], (pixels,))                               # :58
    sampled = valid[indices.to(valid.device)]                                        # :59
    pts = back_project(gt_depth, intrinsics, w2c, sampled, dtype)
    keep = keep_by_keys(pts) if dtype == torch.float32 else keep_by_pixels(sampled, pts)
    pts = pts[keep]                                                                  # :35
    if poses.shape[0] == 0:
        inside = torch.zeros((0, pts.shape[0]), dtype=torch.bool, device=pts.device)
    else:
        inside = project(pts, poses.to(pts.device), intrinsics.to(pts.device), W, H, dtype)[3]
    return {"pixels": sampled, "keep": keep, "pts": pts, "inside": inside, "counts": inside.sum(dim=1).cpu().numpy().astype(np.int64)}


def keyframe_selection_overlap(gt_depth, w2c, intrinsics, keyframe_list, k, pixels=1600, dtype=torch.float32):
    """The whole function (:40-96) through `overlap`: same random streams in the same order, same returned list."""
    poses = torch.stack([kf['est_w2c'] for kf in keyframe_list]) if len(keyframe_list) else torch.zeros((0, 4, 4))
    r = overlap(gt_depth, w2c, intrinsics, poses.to(gt_depth.device), pixels, dtype)
    return list(np.random.permutation(np.array(selection_order(r["counts"])))[:k])    # :93-94


def keyframe_selection_eager(gt_depth, w2c, intrinsics, keyframe_list, k, pixels=1600):
    """The reference's control flow as it runs on a device (:40-96): one small chain of kernels per keyframe, sorted() over 0-dim device
    tensors (one host synchronisation per comparison) and one more per keyframe for `> 0.0`.  fp32.  tools/bench_keyframes.py times it."""
    H, W = gt_depth.shape[1], gt_depth.shape[2]
    valid = valid_pixels(gt_depth)
    indices = torch.randint(valid.shape[0], (pixels,))
    sampled = valid[indices]
    pts = back_project(gt_depth, intrinsics, w2c, sampled)
    pts = pts[keep_by_keys(pts)]
    scored = []
    for kf_id, kf in enumerate(keyframe_list):                                       # :65
        pts4 = torch.cat([pts, torch.ones_like(pts[:, :1])], dim=1)
        cam = (kf['est_w2c'] @ pts4.T).T[:, :3]
        p2d = torch.matmul(intrinsics, cam.transpose(0, 1)).transpose(0, 1)
        zz = p2d[:, 2:] + 1e-5
        p2d = p2d / zz
        uv = p2d[:, :2]
        mask = (uv[:, 0] < W - EDGE) * (uv[:, 0] > EDGE) * (uv[:, 1] < H - EDGE) * (uv[:, 1] > EDGE)
        mask = mask & (zz[:, 0] > 0)
        scored.append((kf_id, mask.sum() / uv.shape[0]))                             # :83
    scored = sorted(scored, key=lambda s: s[1], reverse=True)                        # :88-89
    ids = [kf_id for kf_id, pct in scored if pct > 0.0]                              # :91-92
    return list(np.random.permutation(np.array(ids))[:k])
