#!/usr/bin/env python3
"""Times the multi-scale SSIM of one 1200x680 frame (include/ext/hsr_msssim.h, hsr_utils.evaluate.ms_ssim) with device events, against
  * an eager torch restatement of the same steps on the same device (tests/msssim_ref.py msssim_torch, fp32), and
  * the route the reference takes (utils/eval_helpers.py:1259-1272): mask on the device, copy both images to the host, run the fp32
    restatement there on the host's threads.
One JSON line.  The eager restatement of the same run is the comparison; no speed-up figure is assumed.

    python tools/bench_msssim.py [--calls 200] [--eager-calls 20] [--host-calls 3] [--trace OUTDIR]

--trace OUTDIR takes the kernel launches per call from one `rocprofv3 --kernel-trace --stats` run of its own: a fresh child process
runs the fused path only, writing under OUTDIR.  Numbers not taken are reported as "not measured"."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 680, 1200
WARMUP = 5
SIL_THRES = 0.8


def inputs(dev):
    import msssim_ref as R
    im, gt, depth, opacity, _thres = R.make_frame(H, W, "masked", seed=0)
    return [t.to(dev) for t in (im, gt, depth, opacity)]


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


def measure_fused(calls):
    from hsr_utils import evaluate as E
    im, gt, depth, opacity = inputs(torch.device("cuda:0"))
    us, out = events(lambda: E.ms_ssim(im, gt, depth, opacity, SIL_THRES), calls)
    return {"fused_us": round(us, 1), "fused_score": float(out)}


def measure_restatements(eager_calls, host_calls):
    import msssim_ref as R
    im, gt, depth, opacity = inputs(torch.device("cuda:0"))
    res = {}

    def eager():
        return R.msssim_torch(*R.masked(im, gt, depth, opacity, SIL_THRES), torch.float32)[0]

    def host_route():
        x, y = R.masked(im, gt, depth, opacity, SIL_THRES)
        return R.msssim_torch(x.cpu(), y.cpu(), torch.float32)[0]

    with torch.no_grad():
        if eager_calls > 0:
            us, score = events(eager, eager_calls)
            res.update(torch_eager_device_us=round(us, 1), torch_eager_device_score=score)
        else:
            res["torch_eager_device_us"] = "not measured"
        if host_calls > 0:
            host_route()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(host_calls):
                score = host_route()
            res.update(host_route_ms=round((time.perf_counter() - t0) * 1e3 / host_calls, 2), host_route_score=score,
                       host_threads=torch.get_num_threads())
        else:
            res["host_route_ms"] = "not measured"
    return res


def launches_per_call(outdir, calls):
    if shutil.which("rocprofv3") is None:
        return "not measured (no rocprofv3)"
    os.makedirs(outdir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--", sys.executable, os.path.abspath(__file__),
           "--fused-only", "--calls", str(calls)]
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
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
    ap.add_argument("--eager-calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--fused-only", action="store_true", help="the profiled child: the fused path only, no JSON")
    ap.add_argument("--trace", default=None, help="directory for the rocprofv3 run")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_msssim.py needs a GPU")
    if a.fused_only:
        measure_fused(a.calls)
        return
    res = {"bench": "ms_ssim", "H": H, "W": W, "calls": a.calls}
    res.update(measure_fused(a.calls))
    res.update(measure_restatements(a.eager_calls, a.host_calls))
    res["trace"] = launches_per_call(a.trace, 20) if a.trace else "not measured"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
