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

--tum times the ingest that undistorts the colour image (include/sensor/hsr_frame_undistort.h, hsr_utils.frames.ingest_frame_undistort)
on two frames: a TUM frame, 480x640 with the Freiburg 1 calibration, to itself, and a 680x1200 frame (the default case's sizes, a pinhole
of 600 pixels with Freiburg 1's coefficients) to (680x1200, 340x600, 340x600).  Each is timed, in alternating rounds, against the plain
ingest_frame of the same frame and against the eager chain a caller would write: F.grid_sample (bilinear, zeros outside) of the float
image at a sampling grid built ONCE outside the timed region, F.interpolate to the reduced sizes, / 255, and the depth chain above.  The
eager chain samples at unquantised float32 coordinates, so its colours differ from the 1/32-pixel rule; the distance is reported, not
judged.

    python tools/bench_ingest.py [--scannet | --tum] [--calls 500] [--rounds 7] [--out profiles/ingest_bench.json]"""
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


TUM_FR1 = ((517.3, 516.5, 318.6, 255.3), (0.2624, -0.9531, -0.0054, 0.0026, 1.1633))


def tum_frame(hs, ws, sizes, camera, dist, scale):
    """(undistort, plain, eager) of one frame"""
    from hsr_utils import ingest_frame, ingest_frame_undistort
    g = torch.Generator().manual_seed(0)
    color = torch.randint(0, 256, (hs, ws, 3), generator=g, dtype=torch.uint8).cuda()
    depth = torch.randint(0, 65536, (hs, ws), generator=g, dtype=torch.int32).to(torch.int16).cuda()      # the uint16 words
    index = {hw: ((torch.arange(hw[0], device="cuda") * hs) // hw[0], (torch.arange(hw[1], device="cuda") * ws) // hw[1]) for hw in set(sizes)}
    # the sampling grid, once: the header's source coordinates in float64, then grid_sample's -1..1 with align_corners=True
    fx, fy, cx, cy = camera
    k1, k2, p1, p2, k3 = dist
    v, u = torch.meshgrid(torch.arange(hs, dtype=torch.float64, device="cuda"), torch.arange(ws, dtype=torch.float64, device="cuda"), indexing="ij")
    x, y = (u - cx) / fx, (v - cy) / fy
    r2 = x * x + y * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    us = fx * (x * kr + p1 * 2 * x * y + p2 * (r2 + 2 * x * x)) + cx
    vs = fy * (y * kr + p1 * (r2 + 2 * y * y) + p2 * 2 * x * y) + cy
    grid = torch.stack([2 * us / max(ws - 1, 1) - 1, 2 * vs / max(hs - 1, 1) - 1], dim=-1)[None].float()

    def undistort():
        return ingest_frame_undistort(color, depth, sizes, scale, camera, dist)

    def plain():
        return ingest_frame(color, depth, sizes, scale)

    def eager():
        planar = F.grid_sample(color.permute(2, 0, 1).float()[None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        units = (depth.to(torch.int32) & 0xFFFF).to(torch.float64)
        out = []
        for hw in sizes:
            c = planar[0] if hw == (hs, ws) else F.interpolate(planar, size=hw, mode="bilinear", align_corners=False)[0]
            ys, xs = index[hw]
            out.append((c / 255, (units[ys[:, None], xs[None, :]] / scale).float()[None]))
        return out, None
    return undistort, plain, eager


def report_tum(a):
    frames = {"tum_480x640": (480, 640, [(480, 640)], TUM_FR1[0], TUM_FR1[1], 5000.0),
              "replica_680x1200": (H, W, SIZES, (600.0, 600.0, 599.5, 339.5), TUM_FR1[1], SCALE)}
    result = {"bench": "frame_ingest_undistort", "calls": a.calls, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "frames": {}}
    for name, (hs, ws, sizes, camera, dist, scale) in frames.items():
        runs = dict(zip(("undistort", "plain", "eager"), tum_frame(hs, ws, sizes, camera, dist, scale)))
        for _ in range(WARMUP):
            for run in runs.values():
                run()
        torch.cuda.synchronize()
        rounds, outs = {k: [] for k in runs}, {}
        for _ in range(a.rounds):
            for k, run in runs.items():
                us, outs[k] = events(run, a.calls)
                rounds[k].append(round(us, 1))
        got, base, ref = outs["undistort"][0], outs["plain"][0], outs["eager"][0]
        result["frames"][name] = dict(
            sensor=[hs, ws], sizes=sizes, camera=camera, distortion=dist,
            undistort_us=statistics.median(rounds["undistort"]), plain_ingest_us=statistics.median(rounds["plain"]),
            torch_eager_us=statistics.median(rounds["eager"]), undistort_us_rounds=rounds["undistort"], plain_ingest_us_rounds=rounds["plain"],
            torch_eager_us_rounds=rounds["eager"],
            colour_distance_from_eager_fp32=max(float((f[0] - r[0]).abs().max()) for f, r in zip(got, ref)),
            colour_mean_distance_from_eager_fp32=max(float((f[0] - r[0]).abs().mean()) for f, r in zip(got, ref)),
            depth_equal_to_eager=all(torch.equal(f[1], r[1]) for f, r in zip(got, ref)),
            depth_equal_to_plain_ingest=all(torch.equal(f[1], r[1]) for f, r in zip(got, base)))
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


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
    ap.add_argument("--tum", action="store_true", help="the ingest that undistorts the colour image, against the plain ingest and an eager chain")
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ingest.py needs a GPU")
    if a.scannet and a.tum:
        raise SystemExit("bench_ingest.py: --scannet or --tum, not both")
    if a.tum:
        return report_tum(a)
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
