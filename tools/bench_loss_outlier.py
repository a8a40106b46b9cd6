#!/usr/bin/env python3
"""Times one value + gradient of the outlier-rejecting loss (ignore_outlier_depth_loss = True, scripts/hierslam.py:909-937) on a 680x1200
noisy-depth frame (Gaussian depth noise, about 5 % gross outliers 50 times larger, 3 % holes) with device events, in the tracking form
(colour + depth sums, silhouette on) and in the mapping form (depth mean):
  * fused: hsr_utils.losses.tracking_loss / mapping_depth_loss with ignore_outlier_depth_loss=True (include/ext/hsr_loss_outlier.h);
  * eager: the same loss composed from SlamSession._outlier_mask (torch, with its median) + masked_l1 + weighted_sum,
in the same run, two alternating rounds each (eager, fused, eager, fused).  One JSON line.  No ratio is assumed: the condition reported as
"fused_not_slower" is that the fused time (mean of its rounds) is not above the eager time (mean of its rounds) by more than the spread
between the eager chain's own two rounds.

    python tools/bench_loss_outlier.py [--calls 200] [--trace OUTDIR] [--out FILE]

--trace OUTDIR takes the kernel launches per call from `rocprofv3 --kernel-trace --stats` runs of their own: one fresh child process per
side and form, writing under OUTDIR.  Numbers not taken are reported as "not measured"."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))

H, W = 680, 1200
WARMUP = 10
SIL_THRES = 0.6
WEIGHTS = {"depth": 1.0, "im": 0.5}


def inputs(dev):
    g = torch.Generator().manual_seed(0)
    gt = 0.5 + 4.5 * torch.rand(H, W, generator=g)
    noise = 0.01 * torch.randn(H, W, generator=g)
    noise = torch.where(torch.rand(H, W, generator=g) < 0.05, 50 * noise, noise)
    depth = gt + noise
    gt = torch.where(torch.rand(H, W, generator=g) < 0.03, torch.zeros(()), gt)
    im, gt_im, sil = torch.rand(3, H, W, generator=g), torch.rand(3, H, W, generator=g), torch.rand(1, H, W, generator=g)
    return [t.to(dev).contiguous() for t in (im, gt_im, depth[None], gt[None], sil)]


def make_runs(dev):
    """{(side, form): callable}: one value + gradient each, returning (loss, d depth)"""
    from hsr_utils import losses as L
    from hsr_utils.slam import SlamSession
    im0, gt_im, depth0, gt, sil = inputs(dev)
    im, depth = im0.requires_grad_(True), depth0.requires_grad_(True)

    def done(loss):
        loss.backward()
        out = (loss.detach(), depth.grad)
        im.grad = depth.grad = None
        return out

    def fused_tracking():
        return done(L.tracking_loss(im, gt_im, depth, gt, sil, SIL_THRES, True, WEIGHTS, ignore_outlier_depth_loss=True))

    def eager_tracking():
        mask = SlamSession._outlier_mask(gt, depth.detach()) & (sil > SIL_THRES)
        d, c = L.masked_l1(depth, gt, mask, "sum"), L.masked_l1(im, gt_im, mask, "sum")
        return done(L.weighted_sum((d, c), (WEIGHTS["depth"], WEIGHTS["im"])))

    def fused_mapping():
        return done(L.weighted_sum((L.mapping_depth_loss(depth, gt, ignore_outlier_depth_loss=True),), (WEIGHTS["depth"],)))

    def eager_mapping():
        d = L.masked_l1(depth, gt, SlamSession._outlier_mask(gt, depth.detach()), "mean")
        return done(L.weighted_sum((d,), (WEIGHTS["depth"],)))

    return {("fused", "tracking"): fused_tracking, ("eager", "tracking"): eager_tracking,
            ("fused", "mapping"): fused_mapping, ("eager", "mapping"): eager_mapping}


def events(run, calls):
    for _ in range(WARMUP):
        out = run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        out = run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls, out


def measure(calls):
    runs = make_runs(torch.device("cuda:0"))
    res = {}
    for form in ("tracking", "mapping"):
        us = {"eager": [], "fused": []}
        outs = {}
        for _round in range(2):
            for side in ("eager", "fused"):
                t, outs[side] = events(runs[(side, form)], calls)
                us[side].append(round(t, 1))
        eager, fused = sum(us["eager"]) / 2, sum(us["fused"]) / 2
        spread = abs(us["eager"][0] - us["eager"][1])
        lf, le = float(outs["fused"][0]), float(outs["eager"][0])
        res[form] = {"eager_us_rounds": us["eager"], "fused_us_rounds": us["fused"], "eager_us": round(eager, 1), "fused_us": round(fused, 1),
                     "eager_round_spread_us": round(spread, 1), "fused_not_slower": bool(fused <= eager + spread),
                     "fused_loss": lf, "eager_loss": le, "loss_relative_distance": abs(lf - le) / abs(le),
                     "depth_gradients_differ_at": int((outs["fused"][1] != outs["eager"][1]).sum())}
    return res


def launches_per_call(outdir, side, form, calls):
    if shutil.which("rocprofv3") is None:
        return "not measured (no rocprofv3)"
    outdir = os.path.join(outdir, "%s_%s" % (side, form))
    os.makedirs(outdir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--", sys.executable, os.path.abspath(__file__),
           "--only", "%s,%s" % (side, form), "--calls", str(calls)]
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    if r.returncode != 0:
        return "not measured (rocprofv3 exit %d)" % r.returncode
    files = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return "not measured (no kernel_stats.csv)"
    rows = []
    for row in csv.DictReader(open(files[0])):
        short = row["Name"].replace("(anonymous namespace)::", "").split("(")[0]
        if short:
            rows.append({"kernel": short[:60], "calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2)})
    total = sum(r["calls"] for r in rows)
    return {"launches_per_call": round(total / float(calls + WARMUP), 2), "kernels": sorted(rows, key=lambda r: -r["avg_us"] * r["calls"])[:8]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--only", default=None, help="the profiled child: SIDE,FORM alone, no JSON")
    ap.add_argument("--trace", default=None, help="directory for the rocprofv3 runs")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss_outlier.py needs a GPU")
    if a.only:
        side, form = a.only.split(",")
        events(make_runs(torch.device("cuda:0"))[(side, form)], a.calls)
        return
    res = {"bench": "loss_outlier", "H": H, "W": W, "calls": a.calls, "warmup": WARMUP}
    res.update(measure(a.calls))
    for form in ("tracking", "mapping"):
        res[form]["trace"] = ({side: launches_per_call(a.trace, side, form, 20) for side in ("fused", "eager")} if a.trace else "not measured")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
