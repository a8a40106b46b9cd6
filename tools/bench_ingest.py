#!/usr/bin/env python3
"""Times one ingest of a 1200x680 raw sensor frame (8-bit interleaved colour, 16-bit depth, one class-id image with a 5-level tree) to
the sizes (680x1200, 340x600, 340x600) (include/ext/hsr_frame_ingest.h, hsr_utils.frames.ingest_frame: one launch) with device events,
against the eager chain a caller has to write without it, on the same device: .float() and permute of the colour image,
F.interpolate (bilinear, align_corners=False) to the two reduced sizes, / 255 of all three, integer indexing and a division for the three
depths, and a table gather plus torch.where for the label planes.  All inputs are already on the device in both.  Rounds alternate
between the two so that neither runs on a warmer or a busier device than the other; the median round of each is reported and the rounds
are listed.  One JSON line, also written to --out when given; no speed-up figure is assumed.

--scannet times a ScanNet frame instead (include/ext/hsr_frame_ingest_planes.h, hsr_utils.frames.ingest_frame_planes): colour and labels
968x1296, depth 480x640, to (480x640, 240x320, 240x320) with a 5-level + leaf table, against the same kind of eager chain, each image
indexed from its own size and the last label plane gathered from the table's leaf column.

    python tools/bench_ingest.py [--scannet] [--calls 500] [--rounds 7] [--out profiles/ingest_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))

H, W = 680, 1200
SIZES = [(680, 1200), (340, 600), (340, 600)]
LEVELS, N_IDS = 5, 102
SCALE = 6553.5
WARMUP = 5


def events(run, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        out = run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls, out


def scannet_case():
    """(fused, eager, description) of the ScanNet frame"""
    from hsr_utils import ingest_frame_planes
    (hc, wc), (hd, wd) = (968, 1296), (480, 640)
    sizes = [(480, 640), (240, 320), (240, 320)]
    n_ids, scale = 1358, 1000.0
    g = torch.Generator().manual_seed(0)
    color = torch.randint(0, 256, (hc, wc, 3), generator=g, dtype=torch.uint8).cuda()
    depth = torch.randint(0, 65536, (hd, wd), generator=g, dtype=torch.int32).to(torch.int16).cuda()      # the uint16 words
    labels = torch.randint(0, n_ids + 40, (hc, wc), generator=g, dtype=torch.int32).cuda()                # a few ids beyond the table
    table = torch.randint(-1, 40, (n_ids, LEVELS + 1), generator=g, dtype=torch.int32).cuda()             # five levels, then the leaf

    def nearest(hw, src):
        return (torch.arange(hw[0], device="cuda") * src[0]) // hw[0], (torch.arange(hw[1], device="cuda") * src[1]) // hw[1]
    depth_index = {hw: nearest(hw, (hd, wd)) for hw in set(sizes)}
    label_index = nearest(sizes[0], (hc, wc))

    def fused():
        return ingest_frame_planes(color, depth, sizes, scale, labels=labels, label_table=table, leaf_column=True)

    def eager():
        planar = color.permute(2, 0, 1).float()
        units = (depth.to(torch.int32) & 0xFFFF).to(torch.float64)
        out = []
        for hw in sizes:
            c = F.interpolate(planar[None], size=hw, mode="bilinear", align_corners=False)[0]
            ys, xs = depth_index[hw]
            out.append((c / 255, (units[ys[:, None], xs[None, :]] / scale).float()[None]))
        ys, xs = label_index
        ids = labels[ys[:, None], xs[None, :]].long()
        known = (ids >= 0) & (ids < n_ids)
        rows = table[torch.where(known, ids, 0)].long()                                               # [h, w, L + 1]
        return out, torch.where(known[None], rows.permute(2, 0, 1), ids[None])
    return fused, eager, {"bench": "frame_ingest_planes", "color": [hc, wc], "depth": [hd, wd], "labels": [hc, wc], "sizes": sizes,
                          "label_levels": LEVELS, "leaf_column": True, "n_ids": n_ids}


def report(a, fused, eager, head):
    for _ in range(WARMUP):
        fused(), eager()
    torch.cuda.synchronize()
    rounds = {"fused": [], "eager": []}
    for _ in range(a.rounds):
        us, got = events(fused, a.calls)
        rounds["fused"].append(round(us, 1))
        us, ref = events(eager, a.calls)
        rounds["eager"].append(round(us, 1))
    colour_dist = max(float((f[0] - r[0]).abs().max()) for f, r in zip(got[0], ref[0]))
    result = dict(head, calls=a.calls, rounds=a.rounds,
                  fused_us=statistics.median(rounds["fused"]), torch_eager_us=statistics.median(rounds["eager"]),
                  fused_us_rounds=rounds["fused"], torch_eager_us_rounds=rounds["eager"],
                  colour_distance_from_eager_fp32=colour_dist,
                  depth_equal_to_eager=all(torch.equal(f[1], r[1]) for f, r in zip(got[0], ref[0])),
                  labels_equal_to_eager=bool(torch.equal(got[1], ref[1])), device=torch.cuda.get_device_name(0))
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scannet", action="store_true", help="a ScanNet frame through ingest_frame_planes instead of the default case")
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ingest.py needs a GPU")
    if a.scannet:
        return report(a, *scannet_case())
    from hsr_utils import ingest_frame
    g = torch.Generator().manual_seed(0)
    color = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).cuda()
    depth = torch.randint(0, 65536, (H, W), generator=g, dtype=torch.int32).to(torch.int16).cuda()      # the uint16 words
    labels = torch.randint(0, N_IDS + 4, (H, W), generator=g, dtype=torch.int32).cuda()                 # a few ids beyond the table
    table = torch.randint(-1, 30, (N_IDS, LEVELS), generator=g, dtype=torch.int32).cuda()
    index = {hw: ((torch.arange(hw[0], device="cuda") * H) // hw[0], (torch.arange(hw[1], device="cuda") * W) // hw[1]) for hw in set(SIZES)}

    def fused():
        return ingest_frame(color, depth, SIZES, SCALE, labels=labels, tree_table=table)

    def eager():
        planar = color.permute(2, 0, 1).float()
        units = (depth.to(torch.int32) & 0xFFFF).to(torch.float64)
        out = []
        for hw in SIZES:
            c = planar if hw == (H, W) else F.interpolate(planar[None], size=hw, mode="bilinear", align_corners=False)[0]
            ys, xs = index[hw]
            out.append((c / 255, (units[ys[:, None], xs[None, :]] / SCALE).float()[None]))
        ys, xs = index[SIZES[0]]
        ids = labels[ys[:, None], xs[None, :]].long()
        known = (ids >= 0) & (ids < N_IDS)
        rows = table[torch.where(known, ids, 0)].long()                                               # [h, w, L]
        planes = torch.where(known[None], rows.permute(2, 0, 1), ids[None])
        return out, torch.cat([planes, ids[None]])

    report(a, fused, eager, {"bench": "frame_ingest", "H": H, "W": W, "sizes": SIZES, "label_levels": LEVELS})


if __name__ == "__main__":
    main()
