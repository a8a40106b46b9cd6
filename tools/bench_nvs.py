#!/usr/bin/env python3
"""Times the two device pieces of the novel-view evaluation (include/ext/hsr_view.h) per view, at 1 M Gaussians and 1200x680, isotropic
and anisotropic, against the eager torch chains of the reference's eval_nvs on the same tensors and the same device:

    hsr_view_prep        against utils/eval_helpers.py:1692-1720: the column of ones, the [4,4] @ [4,P] matmul and its slice, for
                         anisotropic maps matrix_to_quaternion, two F.normalize and quat_mult, then the exp, sigmoid and F.normalize
                         (and the tile of the scales) of transformed_params2rendervar;
    evaluate.view_holes  against :1726-1738: the boolean planes, their sum, and the host read of `percent_holes > 0.1` per view.

Device events around `--views` calls after a warm-up; the reference's hole chain ends in a host read, so it is timed with the host clock
around a loop that reads every view (and the fused count with one read after the last view, as evaluate_novel_views makes it).  Both
sides' outputs are compared before anything is timed.  One JSON line.

    python tools/bench_nvs.py [--views 200] [--gaussians 1000000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))

H, W = 680, 1200
SIL_THRES = 0.99


def inputs(P, S, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    params = {"means3D": torch.randn(P, 3, generator=g) * 3, "rgb_colors": torch.rand(P, 3, generator=g),
              "unnorm_rotations": torch.randn(P, 4, generator=g), "logit_opacities": torch.randn(P, 1, generator=g) * 2,
              "log_scales": torch.randn(P, S, generator=g) - 3}
    angle = np.deg2rad(23.0)
    w2c = torch.tensor([[np.cos(angle), 0.0, np.sin(angle), 0.3], [0.0, 1.0, 0.0, -0.2], [-np.sin(angle), 0.0, np.cos(angle), 0.5],
                        [0.0, 0.0, 0.0, 1.0]], dtype=torch.float32)
    return {k: v.to(dev).contiguous() for k, v in params.items()}, w2c.to(dev)


def quat_mult(q1, q2):
    w1, x1, y1, z1 = q1.T
    w2, x2, y2, z2 = q2.T
    return torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                        w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2]).T


def eager_prep(params, w2c):
    """eval_nvs :1692-1712 and transformed_params2rendervar (utils/slam_helpers.py:124-139) in eager torch"""
    from hsr_utils.slam import matrix_to_quaternion
    pts = params['means3D'].detach()
    pts_ones = torch.ones(pts.shape[0], 1).cuda().float()
    pts4 = torch.cat((pts, pts_ones), dim=1)
    means = (w2c @ pts4.T).T[:, :3]
    if params['log_scales'].shape[1] == 1:
        rots = params['unnorm_rotations'].detach()
        scales = torch.tile(torch.exp(params['log_scales']), (1, 3))
    else:
        norm_rots = F.normalize(params['unnorm_rotations'].detach())
        cam_rot = F.normalize(matrix_to_quaternion(w2c[:3, :3]).unsqueeze(0))
        rots = quat_mult(cam_rot, norm_rots)
        scales = torch.exp(params['log_scales'])
    return {'means3D': means, 'rotations': F.normalize(rots), 'opacities': torch.sigmoid(params['logit_opacities']), 'scales': scales,
            'means2D': torch.zeros_like(params['means3D'], requires_grad=True, device="cuda") + 0}


def eager_holes(silhouette, gt_depth):
    """eval_nvs :1726-1738, with its host read"""
    valid_depth_mask = (gt_depth > 0)
    presence_sil_mask = (silhouette > SIL_THRES)
    valid_region_mask = presence_sil_mask | ~valid_depth_mask
    percent_holes = (~valid_region_mask).sum() / valid_region_mask.numel() * 100
    return not bool(percent_holes > 0.1), int((~valid_region_mask).sum())


def device_us(run, views):
    for _ in range(10):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(views):
        run()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / views, 2)


def measure(P, views):
    from hsr_utils import evaluate, slam_helpers as SH
    dev = torch.device("cuda:0")
    res = {}
    for name, S in (("isotropic", 1), ("anisotropic", 3)):
        params, w2c = inputs(P, S, dev)

        def fused():
            return SH.transformed_params2rendervar(params, SH.transform_to_view(params, w2c))
        with torch.no_grad():
            a, b = fused(), eager_prep(params, w2c)
            err = {k: float((a[k] - b[k]).abs().max()) for k in ("means3D", "rotations", "opacities", "scales")}
            res[name] = {"view_prep_us": device_us(fused, views), "eager_chain_us": device_us(lambda: eager_prep(params, w2c), views),
                         "max_abs_difference": err}
        # bytes hsr_view_prep must move per Gaussian: means 12 + rotations 16 + logit 4 + log-scales 4 S in; means 12 + transformed
        # rotations 16 + rotations 16 + opacity 4 + scales 12 out
        nbytes = P * (12 + 16 + 4 + 4 * S + 12 + 16 + 16 + 4 + 12)
        res[name]["view_prep_bytes"] = nbytes
        res[name]["view_prep_GBps_end_to_end"] = round(nbytes / (res[name]["view_prep_us"] * 1e-6) / 1e9, 1)
    g = torch.Generator().manual_seed(1)
    sil = torch.rand(1, H, W, generator=g)
    sil[:, 100:500, 200:900] = 1.0
    depth = torch.rand(1, H, W, generator=g) * 5
    depth[:, :20] = 0
    sil, depth = sil.to(dev), depth.to(dev)
    counts = evaluate.view_holes(sil, depth, SIL_THRES)
    want = eager_holes(sil[0], depth)
    assert int(counts[0]) == want[1], (counts.tolist(), want)
    holes = {"view_holes_us": device_us(lambda: evaluate.view_holes(sil, depth, SIL_THRES), views)}
    for label, run in (("eager_chain_with_host_read_us", lambda: [eager_holes(sil[0], depth) for _ in range(views)]),
                       ("view_holes_one_read_at_the_end_us", lambda: torch.stack([evaluate.view_holes(sil, depth, SIL_THRES) for _ in range(views)]).cpu())):
        run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        holes[label] = round((time.perf_counter() - t0) * 1e6 / views, 2)
    res["holes"] = holes
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--gaussians", type=int, default=1000000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nvs.py needs a GPU")
    res = {"bench": "novel_view", "gaussians": a.gaussians, "H": H, "W": W, "views": a.views}
    res.update(measure(a.gaussians, a.views))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
