#!/usr/bin/env python3
"""Times one step of the replay of a finished run (include/ext/hsr_replay.h) at 1 M Gaussians, K = 26 and K = 0, and a 640x480 view,
against what the same step costs without it, on the same tensors and the same device:

    hsr_replay_select    against (a) the reference's eager chain, viz_scripts/online_recon_sem_replica.py:100-158: the mask, a boolean
                         index per tensor (each ends in a host synchronisation: torch reads the row count), then normalize / sigmoid /
                         exp / tile; and (b) the chain of this package's existing kernels: a byte mask, hsr_compact_append_rows over the
                         six tables (count, scan, row copy), then hsr_view_prep on the copies — called through the C ABI with outputs
                         sized from the plan, so without a host read;
    the K columns        the select's flat copy (lanes along the block's 256 * K floats, destination rows in LDS) against a row per
                         lane, which is what hsr_compact_append_rows's kernel does: select at K = 26 minus select at K = 0, against
                         the compaction of the [P,26] table minus the compaction of a [P,1] table (both differences drop the shared
                         count and scan);
    hsr_replay_cloud     against eager rgbd2pcd (:220-259) up to the device tensors (the reference then copies them to the host as
                         float64), points alone and the 15-byte records.

Device events around `--steps` calls after a warm-up; the eager selection synchronises with the host, so it is also timed with the host
clock.  Outputs are compared before anything is timed.  One JSON line.

    python tools/bench_replay.py [--steps 200] [--gaussians 1000000]
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

H, W = 480, 640
FRAMES = 2000
KEYS = ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales", "semantic")


def inputs(P, K, dev, seed=0):
    """a map whose first third is frame 0's and whose rest arrives in runs, as a run's does; the step shows about two thirds of it"""
    g = torch.Generator().manual_seed(seed)
    params = {"means3D": torch.randn(P, 3, generator=g) * 3, "rgb_colors": torch.rand(P, 3, generator=g),
              "unnorm_rotations": torch.randn(P, 4, generator=g), "logit_opacities": torch.randn(P, 1, generator=g) * 2,
              "log_scales": torch.randn(P, 1, generator=g) - 3, "semantic": torch.randn(P, K, generator=g)}
    ts = torch.zeros(P)
    rest = P - P // 3
    ts[P // 3:] = torch.sort(torch.randint(1, FRAMES, (rest,), generator=g)).values.float()
    return {k: v.to(dev).contiguous() for k, v in params.items()}, ts.to(dev)


def eager_select(params, ts, step, semantic):
    """get_rendervars_semantic (:133-158), with every per-Gaussian tensor selected"""
    idx = ts <= step
    sel = {k: params[k][idx] for k in KEYS if semantic or k != "semantic"}
    log_scales = torch.tile(sel['log_scales'], (1, 3)) if sel['log_scales'].shape[-1] == 1 else sel['log_scales']
    rv = {'means3D': sel['means3D'], 'colors_precomp': sel['rgb_colors'], 'rotations': F.normalize(sel['unnorm_rotations']),
          'opacities': torch.sigmoid(sel['logit_opacities']), 'scales': torch.exp(log_scales),
          'means2D': torch.zeros_like(sel['means3D'], device="cuda")}
    if semantic:
        rv['semantics_precomp'] = sel['semantic']
    return rv


def kernel_chain(params, ts, step, n, semantic, identity):
    """byte mask + hsr_compact_append_rows + hsr_view_prep, outputs sized from the plan (no host read)"""
    from diff_gaussian_rasterization import _abi
    lib, dev = _abi.lib, ts.device
    P = int(ts.numel())
    keep = (ts <= step).to(torch.uint8)
    names = [k for k in KEYS if semantic or k != "semantic"]
    tabs, out = (_abi.hsr_row_table * len(names))(), {}
    for i, k in enumerate(names):
        cols = int(params[k].shape[1])
        out[k] = torch.empty((P, cols), dtype=torch.float32, device=dev)      # the compaction writes at most P rows
        tabs[i] = _abi.hsr_row_table(params[k].data_ptr(), None, out[k].data_ptr(), cols)
    scratch = torch.empty(int(lib.hsr_compact_scratch_bytes(P)), dtype=torch.uint8, device=dev)
    rows = torch.empty(1, dtype=torch.int32, device=dev)
    _abi.call(lib.hsr_compact_append_rows, "hsr_compact_append_rows", dev, P, keep.data_ptr(), 0, len(names), tabs, 0, rows.data_ptr(),
              scratch.data_ptr(), scratch.numel())
    o = dict(dtype=torch.float32, device=dev)
    rv = {'means3D': torch.empty((n, 3), **o), 'rotations': torch.empty((n, 4), **o), 'opacities': torch.empty((n, 1), **o),
          'scales': torch.empty((n, 3), **o)}
    _abi.call(lib.hsr_view_prep, "hsr_view_prep", dev, n, 1, 0, 0 if semantic else 1, out["means3D"].data_ptr(), out["unnorm_rotations"].data_ptr(),
              out["logit_opacities"].data_ptr(), out["log_scales"].data_ptr(), identity.data_ptr(), rv['means3D'].data_ptr(), None,
              rv['rotations'].data_ptr(), rv['opacities'].data_ptr(), rv['scales'].data_ptr())
    rv['colors_precomp'] = out["rgb_colors"][:n]
    if semantic:
        rv['semantics_precomp'] = out["semantic"][:n]
    rv['means2D'] = torch.zeros((n, 3), **o)
    return rv


def compact_one(table, keep):
    from diff_gaussian_rasterization import _abi
    lib, dev = _abi.lib, table.device
    P, cols = int(table.shape[0]), int(table.shape[1])
    dst = torch.empty((P, cols), dtype=torch.float32, device=dev)
    tabs = (_abi.hsr_row_table * 1)(_abi.hsr_row_table(table.data_ptr(), None, dst.data_ptr(), cols))
    scratch = torch.empty(int(lib.hsr_compact_scratch_bytes(P)), dtype=torch.uint8, device=dev)
    rows = torch.empty(1, dtype=torch.int32, device=dev)
    _abi.call(lib.hsr_compact_append_rows, "hsr_compact_append_rows", dev, P, keep.data_ptr(), 0, 1, tabs, 0, rows.data_ptr(), scratch.data_ptr(),
              scratch.numel())
    return dst


def eager_cloud(color, depth, w2c, intrinsics):
    """rgbd2pcd (:220-259) up to the device tensors"""
    width, height = color.shape[2], color.shape[1]
    CX, CY, FX, FY = intrinsics[0][2], intrinsics[1][2], intrinsics[0][0], intrinsics[1][1]
    xx = torch.tile(torch.arange(width).cuda(), (height,))
    yy = torch.repeat_interleave(torch.arange(height).cuda(), width)
    xx = (xx - CX) / FX
    yy = (yy - CY) / FY
    z_depth = depth[0].reshape(-1)
    pts_cam = torch.stack((xx * z_depth, yy * z_depth, z_depth), dim=-1)
    pix_ones = torch.ones(height * width, 1).cuda().float()
    pts4 = torch.cat((pts_cam, pix_ones), dim=1)
    c2w = torch.inverse(w2c)
    pts = (c2w @ pts4.T).T[:, :3]
    cols = torch.permute(color, (1, 2, 0)).reshape(-1, 3)
    return pts.contiguous(), cols.contiguous()


def device_us(run, steps):
    for _ in range(10):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / steps, 2)


def host_us(run, steps):
    for _ in range(5):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        run()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e6 / steps, 2)


def measure(P, steps):
    from hsr_utils import export, replay
    dev = torch.device("cuda:0")
    res = {}
    identity = torch.eye(4, device=dev)
    step = FRAMES // 2
    for K in (26, 0):
        semantic = K > 0
        params, ts = inputs(P, max(K, 1), dev)
        plan = replay.ReplayPlan(ts, FRAMES)
        n = int(plan.counts[step])
        with torch.no_grad():
            a, b, c = replay.replay_rendervars(params, plan, step, semantic=semantic), eager_select(params, ts, step, semantic), \
                kernel_chain(params, ts, step, n, semantic, identity)
            assert a['means3D'].shape[0] == n == b['means3D'].shape[0]
            err = {k: max(float((a[k] - b[k]).abs().max()), float((a[k] - c[k]).abs().max())) for k in a if k != 'means2D'}
            r = {"selected": n, "max_abs_difference": err,
                 "replay_select_us": device_us(lambda: replay.replay_rendervars(params, plan, step, semantic=semantic), steps),
                 "kernel_chain_us": device_us(lambda: kernel_chain(params, ts, step, n, semantic, identity), steps),
                 "eager_chain_us": device_us(lambda: eager_select(params, ts, step, semantic), steps),
                 "eager_chain_host_clock_us": host_us(lambda: eager_select(params, ts, step, semantic), steps),
                 "replay_select_host_clock_us": host_us(lambda: replay.replay_rendervars(params, plan, step, semantic=semantic), steps)}
        # bytes the select must move: the timestep twice, per selected row 36 + 12 (colour) + 4 K in and 44 + 12 + 4 K out (no out_unnorm_rot)
        r["replay_select_bytes"] = 8 * P + n * (36 + 12 + 4 * K + 44 + 12 + 4 * K)
        r["replay_select_GBps_end_to_end"] = round(r["replay_select_bytes"] / (r["replay_select_us"] * 1e-6) / 1e9, 1)
        res["K%d" % K] = r
        if K == 26:
            keep = (ts <= step).to(torch.uint8)
            one = params["logit_opacities"]
            assert torch.equal(compact_one(params["semantic"], keep)[:n], a["semantics_precomp"])
            res["k_columns"] = {"row_per_lane_table26_us": device_us(lambda: compact_one(params["semantic"], keep), steps),
                                "row_per_lane_table1_us": device_us(lambda: compact_one(one, keep), steps)}
    k = res["k_columns"]
    k["flat_copy_us"] = round(res["K26"]["replay_select_us"] - res["K0"]["replay_select_us"], 2)
    k["row_per_lane_copy_us"] = round(k["row_per_lane_table26_us"] - k["row_per_lane_table1_us"], 2)
    # the cloud of a 640x480 view
    g = torch.Generator().manual_seed(2)
    color = torch.rand(3, H, W, generator=g).to(dev)
    depth = (torch.rand(1, H, W, generator=g) * 5 + 0.2).to(dev)
    angle = np.deg2rad(23.0)
    w2c = torch.tensor([[np.cos(angle), 0.0, np.sin(angle), 0.3], [0.0, 1.0, 0.0, -0.2], [-np.sin(angle), 0.0, np.cos(angle), 0.5],
                        [0.0, 0.0, 0.0, 1.0]], dtype=torch.float32, device=dev)
    kmat = np.array([[320.0, 0, 319.5], [0, 320.0, 239.5], [0, 0, 1]], np.float32)
    picture = export.export_frame(im=color)["im"]
    pts, _cols = eager_cloud(color, depth, w2c, kmat)
    got = replay.view_cloud(depth, kmat, w2c)
    res["cloud"] = {"max_abs_difference": float((got - pts).abs().max()),
                    "replay_cloud_points_us": device_us(lambda: replay.view_cloud(depth, kmat, w2c), steps),
                    "replay_cloud_records_us": device_us(lambda: replay.view_cloud(depth, kmat, w2c, picture=picture, records=True), steps),
                    "eager_rgbd2pcd_us": device_us(lambda: eager_cloud(color, depth, w2c, kmat), steps)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--gaussians", type=int, default=1000000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_replay.py needs a GPU")
    res = {"bench": "replay", "gaussians": a.gaussians, "H": H, "W": W, "frames": FRAMES, "steps": a.steps}
    res.update(measure(a.gaussians, a.steps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
