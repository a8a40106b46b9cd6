"""Restatements for the novel-view path (include/ext/hsr_view.h, hsr_utils.evaluate.evaluate_novel_views), written from the lines of the
reference they stand for and from nothing of the code under test:

    transform(params, w2c, rot_source, dtype)      eval_nvs's per-view chain (utils/eval_helpers.py:1692-1712) followed by
                                                   transformed_params2rendervar[_semantic] (utils/slam_helpers.py:124-139, :195-219), in
                                                   torch on the host, in float64 or float32
    matrix_to_quaternion(m)                        the pivot rule of hsr_utils/slam.py:178-196, one matrix at a time, in the dtype given
    build_rotation(q)                              utils/slam_external.py:25-42
    hole_counts(opacity, gt_depth, sil_thres)      :1726-1734 in numpy: (holes, valid-depth pixels)
    nvs_loop(views, ...)                           the loop of eval_nvs in float64 over rendered images that are given
"""
import numpy as np
import torch
import torch.nn.functional as F

import eval_ref

ROT_PARAMS, ROT_TRANSFORMED = 0, 1


def matrix_to_quaternion(m):
    """[3,3] -> [4] (w, x, y, z), real part not negative: the largest of the four pivots decides, the first on ties"""
    one = torch.ones((), dtype=m.dtype)
    pivots = torch.stack([one + m[0, 0] + m[1, 1] + m[2, 2], one + m[0, 0] - m[1, 1] - m[2, 2], one - m[0, 0] + m[1, 1] - m[2, 2],
                          one - m[0, 0] - m[1, 1] + m[2, 2]])
    best = 0
    for k in range(1, 4):
        if pivots[k] > pivots[best]:
            best = k
    rows = [[pivots[0], m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1]],
            [m[2, 1] - m[1, 2], pivots[1], m[1, 0] + m[0, 1], m[0, 2] + m[2, 0]],
            [m[0, 2] - m[2, 0], m[1, 0] + m[0, 1], pivots[2], m[2, 1] + m[1, 2]],
            [m[1, 0] - m[0, 1], m[0, 2] + m[2, 0], m[2, 1] + m[1, 2], pivots[3]]]
    q = torch.stack(rows[best]) / (2.0 * torch.sqrt(pivots[best].clamp_min(1e-12)))
    return -q if q[0] < 0 else q


def build_rotation(q):
    """utils/slam_external.py:25-42 for q [N,4]"""
    norm = torch.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    q = q / norm[:, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rot = torch.zeros((q.size(0), 3, 3), dtype=q.dtype)
    rot[:, 0, 0] = 1 - 2 * (y * y + z * z)
    rot[:, 0, 1] = 2 * (x * y - r * z)
    rot[:, 0, 2] = 2 * (x * z + r * y)
    rot[:, 1, 0] = 2 * (x * y + r * z)
    rot[:, 1, 1] = 1 - 2 * (x * x + z * z)
    rot[:, 1, 2] = 2 * (y * z - r * x)
    rot[:, 2, 0] = 2 * (x * z - r * y)
    rot[:, 2, 1] = 2 * (y * z + r * x)
    rot[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return rot


def quat_mult(q1, q2):
    """utils/slam_helpers.py:21-28"""
    w1, x1, y1, z1 = q1.T
    w2, x2, y2, z2 = q2.T
    w = w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2
    x = w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2
    y = w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2
    z = w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2
    return torch.stack([w, x, y, z]).T


def transform(params, w2c, rot_source, dtype, transform_rots=None):
    """`params`: numpy float32 arrays means3D [P,3], unnorm_rotations [P,4], logit_opacities [P,1], log_scales [P,S]; w2c float32
    [4,4].  The fp32 inputs are converted to `dtype` exactly and everything after is computed in it.  transform_rots: None for the
    reference's rule (S != 1, :1700-1703); the C ABI takes it as an argument of its own, so either branch can be asked for.  Returns
    numpy arrays means3D, unnorm_rotations (transformed_gaussians'), rotations, opacities, scales [P,3]."""
    t = {k: torch.tensor(np.asarray(v, np.float32)).to(dtype) for k, v in params.items()}
    w = torch.tensor(np.asarray(w2c, np.float32)).to(dtype)
    pts = t["means3D"]
    pts4 = torch.cat((pts, torch.ones(pts.shape[0], 1, dtype=dtype)), dim=1)
    means = (w @ pts4.T).T[:, :3]
    S = t["log_scales"].shape[1]
    if (S != 1) if transform_rots is None else transform_rots:
        norm_rots = F.normalize(t["unnorm_rotations"])
        cam_rot = F.normalize(matrix_to_quaternion(w[:3, :3]).unsqueeze(0))
        unnorm = quat_mult(cam_rot, norm_rots)
    else:
        unnorm = t["unnorm_rotations"]
    rotations = F.normalize(t["unnorm_rotations"] if rot_source == ROT_PARAMS else unnorm)
    scales = torch.exp(t["log_scales"])
    if S == 1:
        scales = torch.tile(scales, (1, 3))
    out = dict(means3D=means, unnorm_rotations=unnorm, rotations=rotations, opacities=torch.sigmoid(t["logit_opacities"]), scales=scales)
    return {k: v.numpy() for k, v in out.items()}


def means_bound(params, w2c):
    """per entry of out_means3D: gamma_4 * (|x m0| + |y m1| + |z m2| + |m3|), the rounding bound of three additions of four products,
    gamma_4 = 4u / (1 - 4u), u = 2^-24; evaluated in float64 on the fp32 inputs"""
    u = 2.0 ** -24
    gamma4 = 4 * u / (1 - 4 * u)
    x = np.abs(np.asarray(params["means3D"], np.float64))
    m = np.abs(np.asarray(w2c, np.float64))
    return gamma4 * (x @ m[:3, :3].T + m[:3, 3][None, :])


def hole_counts(opacity, gt_depth, sil_thres):
    """(~(presence | ~valid)).sum() and valid.sum() of utils/eval_helpers.py:1726-1734; sil_thres as the float32 the kernel compares with"""
    with np.errstate(invalid="ignore"):
        presence = np.asarray(opacity, np.float32).reshape(-1) > np.float32(sil_thres)
        valid = np.asarray(gt_depth, np.float32).reshape(-1) > 0
    return int((~(presence | ~valid)).sum()), int(valid.sum())


def nvs_loop(views, sil_thres, mapping_iters, add_new_gaussians):
    """`views`: per scored view (im [3,H,W], depth [1,H,W], opacity [1,H,W], gt_im, gt_depth) as numpy float32, the three first being what
    the renderer gave.  The scores of eval_nvs :1726-1775 in float64 (tests/eval_ref.py frame_metrics: the same lines as the per-frame
    evaluation's), the validity rule with torch's own expression, the averages over the valid views (:1820-1824)."""
    use_sil = mapping_iters == 0 and not add_new_gaussians
    rows, holes, valid = [], [], []
    for im, depth, opac, gt_im, gt_depth in views:
        rows.append(eval_ref.frame_metrics(im, gt_im, depth, gt_depth, opac if use_sil else None, sil_thres if use_sil else None))
        presence = torch.tensor(opac[0]) > sil_thres
        valid_depth = torch.tensor(gt_depth) > 0
        region = presence | ~valid_depth
        percent_holes = (~region).sum() / region.numel() * 100
        holes.append(int((~region).sum()))
        valid.append(not bool(percent_holes > 0.1))
    rows, valid = np.asarray(rows, np.float64), np.asarray(valid)
    out = dict(psnr=rows[:, 0], depth_l1=rows[:, 1], depth_rmse=rows[:, 2], holes=np.asarray(holes, np.int64), valid_nvs_frames=valid)
    for k in ("psnr", "depth_l1", "depth_rmse"):
        out["avg_" + k] = float(out[k][valid].mean()) if valid.any() else float("nan")
    return out
