#!/usr/bin/env python3
"""Times the export of all pictures of one 1200x680 evaluated frame with K = 26 semantic planes in 4 tree levels — rendered and ground-truth
colour, rendered and ground-truth depth through the colour map, the rendered semantic map and the ground-truth level planes coloured per
tree tuple: six pictures, ONE launch (include/ext/hsr_frame_export.h, hsr_utils.export.export_frame) — with device events, against an
eager torch chain that produces the same six uint8 [H,W,3] tensors on the same device: clamp / * 255 / round / permute for the colours,
subtract / divide / clamp / * 255 / truncate / gather for the depths, a softmax and argmax per level, the mixed-radix index and a gather
for the semantic map, range tests, the index and a masked gather for the level planes.  All inputs are already on the device in both.
Rounds alternate between the two so that neither runs on a warmer or a busier device than the other; the median round of each is reported
and the rounds are listed.  Next to the time: the bytes the launch has to move, computed from the shapes (every input read once, 3 bytes
per pixel and picture written; the tables are small and stay in cache), that count over the time, and the bandwidth a streaming kernel
can reach on an MI355X (6.3 TB/s measured with a float4 copy; 8 TB/s is the specification).  One JSON line, also written to --out when
given; no figure is assumed.

    python tools/bench_export.py [--calls 500] [--rounds 7] [--out profiles/export_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))

H, W, K = 680, 1200, 26
SIZES = (3, 5, 8, 10)      # 4 levels, 26 planes, 1200 tuples
LO, HI = 0.0, 6.0
WARMUP = 5
ACHIEVABLE_TBPS = 6.3


def bytes_moved():
    n = H * W
    reads = 2 * 3 * n * 4 + 2 * n * 4 + K * n * 4 + len(SIZES) * n * 8
    writes = 6 * n * 3
    return reads, writes


def events(run, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        out = run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reads, writes = bytes_moved()
    if not torch.cuda.is_available():
        raise SystemExit("bench_export.py needs a GPU (it would move %d bytes per call)" % (reads + writes))
    from hsr_utils import export
    from hsr_utils.export import export_frame, jet_colormap
    g = torch.Generator().manual_seed(0)
    im = (torch.rand(3, H, W, generator=g) * 1.2 - 0.1).cuda()
    gt_im = torch.rand(3, H, W, generator=g).cuda()
    depth = (torch.rand(1, H, W, generator=g) * 7.0).cuda()
    gt_depth = (torch.rand(1, H, W, generator=g) * 7.0).cuda()
    sem = (torch.randn(K, H, W, generator=g) * 3).cuda()
    levels = torch.stack([torch.randint(-1, s, (H, W), generator=g) for s in SIZES]).cuda()      # int64; some -1: outside every level
    n_tuples = 1
    for s in SIZES:
        n_tuples *= s
    table = torch.randint(1, 256, (n_tuples, 3), generator=g, dtype=torch.uint8).cuda()
    jet = jet_colormap("cuda")
    level_sizes = list(SIZES) + [102]
    size_t = [int(s) for s in SIZES]

    def fused():
        return export_frame(im=im, gt_im=gt_im, depth=depth, gt_depth=gt_depth, im_semantic=sem, gt_levels=levels, level_sizes=level_sizes,
                            tuple_table=table, depth_table=jet, depth_range=(LO, HI))

    def colour(x):
        return (x.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()

    def depth_picture(d):
        return jet[(((d[0] - LO) / (HI - LO)).clamp(0, 1) * 255).to(torch.int64)]

    def eager():
        idx, begin = torch.zeros((H, W), dtype=torch.int64, device="cuda"), 0
        for s in size_t:
            idx = idx * s + torch.softmax(sem[begin:begin + s], dim=0).argmax(dim=0)
            begin += s
        ok, gidx = torch.ones((H, W), dtype=torch.bool, device="cuda"), torch.zeros((H, W), dtype=torch.int64, device="cuda")
        for plane, s in zip(levels, size_t):
            ok = ok & (plane >= 0) & (plane < s)
            gidx = gidx * s + plane.clamp(0, s - 1)
        return {"im": colour(im), "gt_im": colour(gt_im), "depth": depth_picture(depth), "gt_depth": depth_picture(gt_depth),
                "im_semantic": table[idx], "gt_levels": table[gidx] * ok[..., None]}

    # the entry point alone, as export_frame calls it: its arguments are recorded from one call (whose outputs are kept alive) and replayed,
    # so that back-to-back launches are limited by the kernel and not by the wrapper's allocations
    recorded, entry = [], export._lib.hsr_frame_export
    export._lib.hsr_frame_export = lambda *args: recorded.append(args) or entry(*args)
    kept = fused()
    export._lib.hsr_frame_export = entry

    def launch():
        entry(*recorded[0])
        return kept

    for _ in range(WARMUP):
        fused(), eager(), launch()
    torch.cuda.synchronize()
    rounds = {"fused": [], "eager": [], "launch": []}
    for _ in range(a.rounds):
        us, _kept = events(launch, a.calls)
        rounds["launch"].append(round(us, 1))
        us, got = events(fused, a.calls)
        rounds["fused"].append(round(us, 1))
        us, ref = events(eager, a.calls)
        rounds["eager"].append(round(us, 1))
    fused_us, launch_us = statistics.median(rounds["fused"]), statistics.median(rounds["launch"])
    result = {"bench": "frame_export", "H": H, "W": W, "K": K, "level_sizes": list(SIZES), "pictures": sorted(got), "calls": a.calls,
              "rounds": a.rounds, "fused_us": fused_us, "torch_eager_us": statistics.median(rounds["eager"]),
              "launch_us": launch_us, "fused_us_rounds": rounds["fused"], "torch_eager_us_rounds": rounds["eager"],
              "launch_us_rounds": rounds["launch"], "bytes_read": reads, "bytes_written": writes,
              "launch_TB_per_s": round((reads + writes) / (launch_us * 1e-6) / 1e12, 3), "achievable_TB_per_s_streaming": ACHIEVABLE_TBPS,
              "share_of_achievable": round((reads + writes) / (launch_us * 1e-6) / 1e12 / ACHIEVABLE_TBPS, 3),
              "note": "fused_us: export_frame, wrapper included; launch_us: back-to-back calls of hsr_frame_export with recorded arguments "
                      "(kernel plus launch gap; the inputs, 137 MB, fit the 256 MB Infinity Cache, so repeated calls may read from it "
                      "rather than from HBM)",
              "pixels_differing_from_eager": {k: int((got[k] != ref[k]).any(dim=-1).sum()) for k in sorted(got)},
              "device": torch.cuda.get_device_name(0)}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
