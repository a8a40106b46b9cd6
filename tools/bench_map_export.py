#!/usr/bin/env python3
"""Times the export of the map as a semantic PLY (59-byte records coloured per tree tuple: include/ext/hsr_map_export.h,
hsr_utils.map_export) for 1 M and 4 M Gaussians at K = 26 with levels (4, 8, 14), and 1 M at K = 102 with levels (3, 5, 9, 17, 68):

  (a) launch   the hsr_map_export launch alone: its arguments are recorded from one export_map call (whose tensors are kept alive) and
               replayed back to back between two device events; the median round is reported and the rounds are listed;
  copy         in the same rounds, a device-to-device copy that moves as many bytes as the launch reads plus writes (a copy of n bytes
               reads n and writes n, so n is half that sum): what a kernel with no LDS round trip and no 59-byte records takes;
  (b) file     save_map_ply_semantic end to end, wall clock around a synchronised call: the table, the launch, one device-to-host copy
               of the body, one write;
  (c) host     the way to the same file without this module: .cpu() of every array, map_io.transfer_tree_label, a numpy table lookup,
               map_io.save_ply_semantic.  The two files are compared byte for byte (the logits lie on a grid of 1/64, so that numpy's
               argmax and the fp32 softmax rule agree).

Bytes are computed from the shapes (every input read once; the table is small and stays in cache).  One JSON line per case, also
appended to --out when given; no figure is assumed.

    python tools/bench_map_export.py [--calls 50] [--rounds 7] [--files 3] [--out profiles/map_export_bench.json] [--dir DIR]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))

CASES = ((1 << 20, 26, (4, 8, 14)), (1 << 22, 26, (4, 8, 14)), (1 << 20, 102, (3, 5, 9, 17, 68)))
WARMUP = 3


def bytes_moved(P, K):
    reads = P * 4 * (3 + 4 + 1 + 1 + K)      # means3D, unnorm_rotations, logit_opacities, log_scales [P,1], semantic
    return reads, P * 59


def events(run, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def wall(run, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append(round((time.perf_counter() - t0) * 1e3, 2))
    return times


def spread(values):
    return round((max(values) - min(values)) / statistics.median(values), 3)


def case(P, K, sizes, a, folder):
    from hsr_utils import map_export, map_io
    from hsr_utils.export import tuple_colour_table
    g = torch.Generator().manual_seed(P + K)
    params = {"means3D": torch.randn(P, 3, generator=g), "rgb_colors": torch.rand(P, 3, generator=g),
              "unnorm_rotations": torch.randn(P, 4, generator=g), "logit_opacities": torch.randn(P, 1, generator=g),
              "log_scales": torch.randn(P, 1, generator=g) - 4,
              "semantic": torch.randint(-128, 129, (P, K), generator=g).float() / 64}
    params = {k: v.cuda() for k, v in params.items()}
    level_sizes = list(sizes) + [K]
    n_tuples = int(np.prod(sizes))
    rng = np.random.default_rng(0)
    colour_map = {tuple(int(v) for v in np.unravel_index(i, sizes)): tuple(int(c) for c in rng.integers(1, 256, size=3))
                  for i in rng.choice(n_tuples, size=min(n_tuples, 200), replace=False)}
    table = tuple_colour_table(colour_map, level_sizes, False, "cuda")

    recorded, entry = [], map_export._lib.hsr_map_export
    map_export._lib.hsr_map_export = lambda *args: recorded.append(args) or entry(*args)
    kept = map_export.export_map(params, colour="tree", table=table, level_sizes=level_sizes)
    map_export._lib.hsr_map_export = entry
    reads, writes = bytes_moved(P, K)
    src = torch.empty((reads + writes) // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def launch():
        entry(*recorded[0])

    def copy():
        dst.copy_(src)

    for _ in range(WARMUP):
        launch(), copy()
    torch.cuda.synchronize()
    rounds = {"launch": [], "copy": []}
    for _ in range(a.rounds):
        rounds["launch"].append(round(events(launch, a.calls), 1))
        rounds["copy"].append(round(events(copy, a.calls), 1))
    launch_us, copy_us = statistics.median(rounds["launch"]), statistics.median(rounds["copy"])

    mine, theirs = os.path.join(folder, "device.ply"), os.path.join(folder, "host.ply")

    def device_file():
        map_export.save_map_ply_semantic(mine, params, colour_map, level_sizes, wildcard=False)

    def host_file():
        host = {k: v.cpu().numpy() for k, v in params.items()}
        labels = map_io.transfer_tree_label(host["semantic"], level_sizes)
        idx = np.zeros(P, dtype=np.int64)
        for lab, s in zip(labels, sizes):
            idx = idx * s + lab
        map_io.save_ply_semantic(theirs, host["means3D"], host["log_scales"], host["unnorm_rotations"], host_table[idx],
                                 host["logit_opacities"])

    host_table = table.cpu().numpy()
    device_file()      # warm-up: the page cache of the target, the pinned staging of the copy
    file_ms = wall(device_file, a.files)
    host_ms = wall(host_file, a.files)
    with open(mine, "rb") as f1, open(theirs, "rb") as f2:
        equal = f1.read() == f2.read()
    size = os.path.getsize(mine)
    os.remove(mine), os.remove(theirs)
    del kept
    return {"bench": "map_export", "P": P, "K": K, "level_sizes": list(sizes), "calls": a.calls, "rounds": a.rounds,
            "bytes_read": reads, "bytes_written": writes,
            "launch_us": launch_us, "launch_us_rounds": rounds["launch"], "launch_spread": spread(rounds["launch"]),
            "copy_us": copy_us, "copy_us_rounds": rounds["copy"], "copy_spread": spread(rounds["copy"]), "copy_bytes_each_way": src.numel(),
            "launch_over_copy": round(launch_us / copy_us, 2), "launch_TB_per_s": round((reads + writes) / (launch_us * 1e-6) / 1e12, 3),
            "file_ms": statistics.median(file_ms), "file_ms_runs": file_ms, "host_way_ms": statistics.median(host_ms), "host_way_ms_runs": host_ms,
            "host_way_over_file": round(statistics.median(host_ms) / statistics.median(file_ms), 1), "file_bytes": size,
            "files_equal": equal, "device": torch.cuda.get_device_name(0),
            "note": "launch_us: back-to-back hsr_map_export calls with recorded arguments (kernel plus launch gap); copy_us: torch's "
                    "device-to-device copy of copy_bytes_each_way bytes, the same bytes moved; file_ms and host_way_ms: wall clock, the "
                    "file written to the directory given (a temporary one by default)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--files", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_map_export.py needs a GPU")
    lines = []
    with tempfile.TemporaryDirectory(dir=a.dir) as folder:
        for P, K, sizes in CASES:
            line = json.dumps(case(P, K, sizes, a, folder))
            print(line, flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
