#!/usr/bin/env python3
"""The optimizer step of a Hier-SLAM iteration (scripts/hierslam.py:1852, :2053) and the tracking loop's best-pose bookkeeping
(:1855-1860).  One JSON line with device-event times:

  step_headline   one Adam step over the headline map (P Gaussians, K semantic planes, camera tensors of T frames, every map gradient
                  dense) for K = 26 and 102: torch's default (foreach), fused=True, foreach=False and hsr_utils.optim.Adam, with the
                  algorithmic traffic (read p, g, m, v; write p, m, v: 28 B per element) and the achieved rate
  step_tracking   the tracking optimizer (configs/replica lrs: the map at lr 0, the pose at 4e-4 / 2e-3) with the map attached, as the
                  reference runs it (means3D detached, the other map tensors get gradients), and with the map detached
  tracking_loop   ~100 tracking iterations at 1200x680: fused prep, render, losses.tracking_loss, backward, step, and the best-pose
                  rule: the reference's host compare (`if loss < current_min_loss`) or TrackingCandidate; wall time per iteration

    python tools/bench_optim.py [--P 500000] [--steps 200] [--loop-iters 100] [--only step|tracking|loop]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))

COPY_RATE = 6.3e12     # float4 copy rate of the MI355X (bytes/s), the bound of a streaming kernel


def _map(P, K, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    shapes = {"means3D": (P, 3), "rgb_colors": (P, 3), "unnorm_rotations": (P, 4), "logit_opacities": (P, 1), "log_scales": (P, 1),
              "semantic": (P, K), "cam_unnorm_rots": (1, 4, T), "cam_trans": (1, 3, T)}
    return {k: torch.randn(s, generator=g).cuda().requires_grad_(True) for k, s in shapes.items()}


def _set_grads(params, names, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for k, p in params.items():
        p.grad = torch.randn(p.shape, generator=g, device="cuda") * 1e-3 if k in names else None


def _time_steps(opt, steps):
    """device-event time of one step, averaged over `steps` steps after a warm-up of every shape"""
    for _ in range(5):
        opt.step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        opt.step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def _variants():
    from hsr_utils.optim import Adam
    return {"torch_foreach_default": lambda g, **kw: torch.optim.Adam(g, **kw),
            "torch_fused": lambda g, **kw: torch.optim.Adam(g, fused=True, **kw),
            "torch_single_tensor": lambda g, **kw: torch.optim.Adam(g, foreach=False, **kw),
            "hsr": lambda g, **kw: Adam(g, **kw)}


def step_headline(P, T, steps):
    out = {}
    lrs = {"means3D": 1e-4, "rgb_colors": 2.5e-3, "unnorm_rotations": 1e-3, "logit_opacities": 0.05, "log_scales": 1e-3, "semantic": 2.5e-3,
           "cam_unnorm_rots": 0.0, "cam_trans": 0.0}
    for K in (26, 102):
        params = _map(P, K, T)
        _set_grads(params, set(params))
        numel = sum(p.numel() for p in params.values())
        row = {"elements": numel, "bytes": 28 * numel, "bound_ms_at_copy_rate": 28 * numel / COPY_RATE * 1e3}
        for name, make in _variants().items():
            ps = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
            for k in ps:
                ps[k].grad = params[k].grad
            opt = make([{"params": [ps[k]], "name": k, "lr": lrs[k]} for k in ps], lr=0.0, eps=1e-15)   # hierslam.py:417
            ms = _time_steps(opt, steps)
            row[name] = {"ms": ms, "TB_s": 28 * numel / (ms * 1e-3) / 1e12}
            if name == "hsr":
                row[name]["fused_tensors"] = opt.last_fused_tensors
            del opt, ps
            torch.cuda.empty_cache()
        out["K%d" % K] = row
        del params
        torch.cuda.empty_cache()
    return out


def step_tracking(P, T, steps):
    lrs = {"means3D": 0.0, "rgb_colors": 0.0, "unnorm_rotations": 0.0, "logit_opacities": 0.0, "log_scales": 0.0, "semantic": 0.0,
           "cam_unnorm_rots": 4e-4, "cam_trans": 2e-3}     # configs/replica/hierslam_semantic_run.py:85-94
    params = _map(P, 26, T)
    out = {}
    for case, names in (("map_attached_lr0", set(params) - {"means3D"}), ("map_detached", {"cam_unnorm_rots", "cam_trans"})):
        _set_grads(params, names)
        numel = sum(params[k].numel() for k in names)
        row = {"elements": numel, "bytes": 28 * numel}
        for name, make in _variants().items():
            if name != "hsr" and name != "torch_foreach_default":
                continue
            ps = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
            for k in ps:
                ps[k].grad = params[k].grad
            opt = make([{"params": [ps[k]], "name": k, "lr": lrs[k]} for k in ps])    # hierslam.py:415
            ms = _time_steps(opt, steps)
            row[name] = {"ms": ms, "TB_s": 28 * numel / (ms * 1e-3) / 1e12}
            del opt, ps
            torch.cuda.empty_cache()
        out[case] = row
    return out


def tracking_loop(P, iters, W=1200, H=680):
    from diff_gaussian_rasterization import GaussianRasterizer_semantic
    from hsr_utils import slam_helpers as SH, losses as L, setup_camera, make_scene
    from hsr_utils.camera import replica_intrinsics
    from hsr_utils.optim import Adam, TrackingCandidate
    K = 26
    kmat = replica_intrinsics(W, H)
    cam = setup_camera(W, H, kmat, np.eye(4), device="cuda")
    sc = make_scene(P, W, H, K, kmat, seed=0)
    g = torch.Generator().manual_seed(0)
    base = {"means3D": sc["means3D"], "unnorm_rotations": sc["rotations"], "logit_opacities": torch.logit(sc["opacities"].clamp(1e-4, 1 - 1e-4)),
            "log_scales": sc["scales"][:, :1].log(), "rgb_colors": sc["colors_precomp"], "semantic": sc["semantics_precomp"]}
    base = {k: v.clone().cuda() for k, v in base.items()}
    rots = torch.zeros(1, 4, 4); rots[0, 0] = 1.0
    base["cam_unnorm_rots"], base["cam_trans"] = rots.cuda(), torch.zeros(1, 3, 4).cuda()
    gt_im, gt_d = torch.rand(3, H, W, generator=g).cuda(), (torch.rand(1, H, W, generator=g) * 5 + 0.5).cuda()
    lrs = {"means3D": 0.0, "rgb_colors": 0.0, "unnorm_rotations": 0.0, "logit_opacities": 0.0, "log_scales": 0.0, "semantic": 0.0,
           "cam_unnorm_rots": 4e-4, "cam_trans": 2e-3}
    tidx = 1

    def run(opt_cls, device_candidate, n):
        params = {k: v.clone().requires_grad_(True) for k, v in base.items()}
        opt = opt_cls([{"params": [v], "name": k, "lr": lrs[k]} for k, v in params.items()])
        cand = TrackingCandidate(params, tidx) if device_candidate else None
        best = float(1e20)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            rv = SH.transformed_params2rendervar_semantic(params, SH.transform_to_frame(params, tidx, False, True))
            im, radius, sem, depth, med, opac = GaussianRasterizer_semantic(raster_settings=cam)(**rv)
            loss = L.tracking_loss(im, gt_im, depth, gt_d, opac, sil_thres=0.99, loss_weights={"im": 0.5, "depth": 1.0})
            loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
            with torch.no_grad():
                if cand is not None:
                    cand.update(loss)
                elif loss < best:                                   # scripts/hierslam.py:1855-1860
                    best = loss
                    _r = params["cam_unnorm_rots"][..., tidx].detach().clone()
                    _t = params["cam_trans"][..., tidx].detach().clone()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    out = {"workload": "tracking iteration %dx%d, P=%d, K=%d, map attached at lr 0 (the reference)" % (W, H, P, K)}
    cases = (("torch_adam_host_compare", torch.optim.Adam, False), ("hsr_adam_host_compare", Adam, False),
             ("hsr_adam_tracking_candidate", Adam, True))
    for name, cls, dc in cases:
        run(cls, dc, 5)
    for rnd in range(2):                                            # two alternating rounds
        for name, cls, dc in cases:
            out.setdefault(name + "_ms_per_iter", []).append(run(cls, dc, iters))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=500000)
    ap.add_argument("--T", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--loop-iters", type=int, default=100)
    ap.add_argument("--only", choices=("step", "tracking", "loop"), default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_optim.py measures on the GPU"
    res = {"device": torch.cuda.get_device_name(0)}
    if a.only in (None, "step"):
        res["step_headline"] = step_headline(a.P, a.T, a.steps)
    if a.only in (None, "tracking"):
        res["step_tracking"] = step_tracking(a.P, a.T, a.steps)
    if a.only in (None, "loop"):
        res["tracking_loop"] = tracking_loop(a.P, a.loop_iters)
    print(json.dumps(res))
