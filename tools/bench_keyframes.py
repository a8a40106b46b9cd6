#!/usr/bin/env python3
"""Times one keyframe selection (include/hsr_keyframes.h, hsr_utils/keyframes.py keyframe_selection_overlap) at 1200x680 with 1600
sampled pixels and 50, 200 and 400 keyframes, against the eager chain on the same device in the same run: tests/keyframe_ref.py's
keyframe_selection_eager, the reference's control flow (one chain of small kernels per keyframe, sorted() over 0-dim device tensors,
one host compare per keyframe).  Wall time per call and device-event time per call for both; one JSON line.

    python tools/bench_keyframes.py [--calls 30] [--eager-calls 3] [--trace OUTDIR]

--trace OUTDIR adds the kernel launches per call: fresh child processes run one path each under `rocprofv3 --kernel-trace --stats`, in
runs of their own, writing under OUTDIR.  Numbers not taken are reported as "not measured"."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W, PIXELS, K_SELECT = 680, 1200, 1600, 22        # mapping_window_size 24 (configs/replica) - 2
SIZES = (50, 200, 400)


def _rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    x, y, z = axis
    Kx = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def inputs(n_kf, dev):
    g = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (2.5 + 0.8 * np.sin(5.0 * xx / W + 1.0) + 0.6 * np.cos(3.0 * yy / H)).astype(np.float32)
    depth[g.random((H, W)) < 0.1] = 0.0
    K = np.array([[600.0, 0, 599.5], [0, 600.0, 339.5], [0, 0, 1]], np.float32)
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = _rot([0.2, 1.0, 0.1], 0.4), [0.1, -0.2, 0.3]
    poses = []
    for i in range(n_kf):
        a = 2 * np.pi * i / n_kf
        rel = np.eye(4)
        rel[:3, :3], rel[:3, 3] = _rot([0.1 * np.sin(3 * a), 1.0, 0.05], a), [0.8 * np.sin(a), 0.1 * np.cos(2 * a), 0.5 * (1 - np.cos(a))]
        poses.append(torch.tensor((rel @ w2c).astype(np.float32), device=dev))
    t = lambda m: torch.tensor(np.asarray(m, np.float32), device=dev)
    return t(depth[None]), t(w2c), t(K), [{'id': 5 * i, 'est_w2c': m} for i, m in enumerate(poses)]


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(calls):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls, e0.elapsed_time(e1) / calls, out


def run_path(path, n_kf, calls, warmup):
    import keyframe_ref as R
    from hsr_utils import keyframes as KF
    dev = torch.device("cuda:0")
    depth, w2c, K, kfl = inputs(n_kf, dev)
    if path == "fused":
        table = KF.KeyframePoses(device=dev)
        for kf in kfl:
            table.append(kf['est_w2c'])
        fn = lambda: KF.keyframe_selection_overlap(depth, w2c, K, table, K_SELECT, PIXELS)
    else:
        fn = lambda: R.keyframe_selection_eager(depth, w2c, K, kfl, K_SELECT, PIXELS)

    def seeded():
        torch.manual_seed(1)
        np.random.seed(1)
        return fn()
    with torch.no_grad():
        return timed(seeded, calls, warmup)


def launches(outdir, path, n_kf, calls):
    if shutil.which("rocprofv3") is None:
        return "not measured (no rocprofv3)"
    d = os.path.join(outdir, "%s_%d" % (path, n_kf))
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--child", path, "--child-kf", str(n_kf), "--calls", str(calls)]
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    if r.returncode != 0:
        return "not measured (rocprofv3 exit %d)" % r.returncode
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return "not measured (no kernel_stats.csv)"
    total = sum(int(row["Calls"]) for row in csv.DictReader(open(files[0])))
    return round(total / calls, 1)       # the child makes no warm-up call; building the inputs adds a few launches, spread over the calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--eager-calls", type=int, default=3)
    ap.add_argument("--trace", default=None, help="directory for the rocprofv3 runs")
    ap.add_argument("--child", default=None, help="the profiled child: one path, no JSON")
    ap.add_argument("--child-kf", type=int, default=400)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_keyframes.py needs a GPU")
    if a.child:
        run_path(a.child, a.child_kf, a.calls, 0)
        return
    res = {"bench": "keyframe_selection", "H": H, "W": W, "pixels": PIXELS, "k": K_SELECT, "calls": a.calls, "eager_calls": a.eager_calls}
    for n_kf in SIZES:
        wall, dev_ms, sel = run_path("fused", n_kf, a.calls, 5)
        r = {"fused_wall_ms": round(wall, 3), "fused_device_ms": round(dev_ms, 3), "fused_selected": [int(i) for i in sel]}
        if a.eager_calls > 0:
            wall, dev_ms, ref = run_path("eager", n_kf, a.eager_calls, 1)
            r.update(eager_wall_ms=round(wall, 2), eager_device_ms=round(dev_ms, 2), same_selection=[int(i) for i in ref] == r["fused_selected"])
        else:
            r.update(eager_wall_ms="not measured", eager_device_ms="not measured")
        if a.trace:
            r["fused_launches_per_call"] = launches(a.trace, "fused", n_kf, 20)
            r["eager_launches_per_call"] = launches(a.trace, "eager", n_kf, 2) if n_kf != 200 else "not measured"
        else:
            r["fused_launches_per_call"] = r["eager_launches_per_call"] = "not measured"
        res["kf_%d" % n_kf] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
