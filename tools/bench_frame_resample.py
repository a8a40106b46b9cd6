#!/usr/bin/env python3
"""Times the device resample of one 1200x680 RGB-D frame to two 600x340 levels (include/ext/hsr_frame_resample.h,
hsr_utils.slam.resample_frame: one launch) with device events, against the eager chain of F.interpolate calls that produces the same
four tensors on the same device (bilinear with align_corners=False for the colours, nearest for the depths).  One JSON line; the eager
chain of the same run is the comparison, no speed-up figure is assumed.

    python tools/bench_frame_resample.py [--calls 2000]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))

H, W = 680, 1200
SIZES = [(340, 600), (340, 600)]
WARMUP = 5


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frame_resample.py needs a GPU")
    from hsr_utils import resample_frame
    g = torch.Generator().manual_seed(0)
    color = torch.rand(3, H, W, generator=g).cuda()
    depth = (torch.rand(1, H, W, generator=g) * 5 + 0.5).cuda()

    def eager():
        return [(F.interpolate(color[None], size=hw, mode="bilinear", align_corners=False)[0], F.interpolate(depth[None], size=hw, mode="nearest")[0])
                for hw in SIZES]
    fused_us, fused = events(lambda: resample_frame(color, depth, SIZES), a.calls)
    eager_us, ref = events(eager, a.calls)
    colour_dist = max(float((f[0] - r[0]).abs().max()) for f, r in zip(fused, ref))
    depth_equal = all(torch.equal(f[1], r[1]) for f, r in zip(fused, ref))
    print(json.dumps({"bench": "frame_resample", "H": H, "W": W, "sizes": SIZES, "calls": a.calls, "fused_us": round(fused_us, 1),
                      "torch_eager_us": round(eager_us, 1), "colour_distance_from_eager_fp32": colour_dist, "depth_equal_to_eager": depth_equal}))


if __name__ == "__main__":
    main()
