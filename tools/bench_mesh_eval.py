#!/usr/bin/env python3
"""Measures the nearest-neighbour search of the mesh evaluation on the device (include/eval/hsr_mesh_eval.h; EXPERIMENTS.md §20): N
samples against N samples (default 200 000) of the room that tools/bench_mesh.py meshes, drawn with two seeds.  The grid path: the build
step by step (cells / sort / ranges / pack) and as NearestGrid does it, and the query in each direction.  The comparison is the eager
chain a user would write today on the same device: chunked torch.cdist + min, and the same chain with the squared distance written out
((dx*dx + dy*dy) + dz*dz, then min), whose values and indices must equal the grid's bit for bit at this size.  Times are device events
around warmed-up work, the two paths alternating within this one call; one JSON line per measurement, and all of them in --out.

    python tools/bench_mesh_eval.py [--samples N] [--reps R] [--eager-reps R] [--chunk C] [--out JSON]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def room_mesh(views_n, dev):
    """the room of tools/bench_mesh.py fused into its 256^3 volume and extracted: (vertices, faces, labels)"""
    import numpy as np
    import bench_mesh as B
    from hsr_utils import mesh
    k = np.array([[B.FX, 0, B.W / 2 - 0.5], [0, B.FX, B.H / 2 - 0.5], [0, 0, 1]], np.float32)
    poses = [B.rotation(ax, ay) for ax in (-0.5, 0.0, 0.5) for ay in np.linspace(0, 2 * np.pi, max(1, views_n // 3), endpoint=False)]
    dims, h = (256, 256, 256), 0.02
    vol = mesh.TsdfVolume(tuple(-h * (d - 1) / 2 for d in dims), dims, h, labels=True)
    for p in poses:
        depth, colour, labels = B.room_view(p, dev)
        vol.integrate(depth, p, k, color=colour, labels=labels)
    vertices, faces, _rgb, labels = vol.extract()
    return vertices, faces, labels


def event_ms(fn, batch=1):
    """(milliseconds per call, the last result): device events around `batch` back-to-back calls"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / batch, out


def eager_cdist(q, p, chunk):
    """chunked torch.cdist + min: (distance, index)"""
    import torch
    d, i = [], []
    for s in range(0, q.shape[0], chunk):
        m = torch.cdist(q[s:s + chunk], p).min(dim=1)
        d.append(m.values)
        i.append(m.indices)
    return torch.cat(d), torch.cat(i)


def eager_exact(q, p, chunk):
    """the same chain with the header's squared distance written out: (d2, index), comparable bit for bit"""
    import torch
    px, py, pz = p[:, 0][None], p[:, 1][None], p[:, 2][None]
    d, i = [], []
    for s in range(0, q.shape[0], chunk):
        c = q[s:s + chunk]
        dx, dy, dz = c[:, 0:1] - px, c[:, 1:2] - py, c[:, 2:3] - pz
        m = ((dx * dx + dy * dy) + dz * dz).min(dim=1)
        d.append(m.values)
        i.append(m.indices)
    return torch.cat(d), torch.cat(i)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=20, help="timed rounds of the grid path")
    ap.add_argument("--batch", type=int, default=20, help="back-to-back calls of a grid step inside one timed window")
    ap.add_argument("--eager-reps", type=int, default=3, help="of those rounds, how many also time the eager chains")
    ap.add_argument("--chunk", type=int, default=2048, help="queries per chunk of the eager chains")
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_eval.py needs a GPU")
    from diff_gaussian_rasterization import _abi
    from hsr_utils import mesh_eval
    dev = torch.device("cuda", torch.cuda.current_device())
    lib, n = _abi.lib, a.samples
    results = []

    def report(**kw):
        results.append(kw)
        print(json.dumps(kw), flush=True)

    vertices, faces, labels = room_mesh(a.views, dev)
    ms_sample, (pa, _fa, _la) = event_ms(lambda: mesh_eval.sample_mesh(vertices, faces, n, 0, labels))
    ms_sample, (pa, _fa, _la) = event_ms(lambda: mesh_eval.sample_mesh(vertices, faces, n, 0, labels))      # warmed up
    pb = mesh_eval.sample_mesh(vertices, faces, n, 1, labels)[0]
    area = float(mesh_eval.face_areas(vertices, faces).double().sum())
    cell = 2.0 * np.sqrt(area / n)
    report(what="room", vertices=int(vertices.shape[0]), faces=int(faces.shape[0]), area_m2=round(area, 3), samples=n, cell_m=round(cell, 5),
           sample_ms=round(ms_sample, 3))

    # ---- the build, step by step on grid B's arguments, and as one constructor (which adds the host read of the box) ----
    grid = {"a": mesh_eval.NearestGrid(pa, cell), "b": mesh_eval.NearestGrid(pb, cell)}
    g = grid["b"]
    X, Y, Z = g.dims
    cells = torch.empty(n, dtype=torch.int32, device=dev)
    packed = torch.empty((n, 4), dtype=torch.float32, device=dev)
    ids = torch.arange(X * Y * Z + 1, dtype=torch.int32, device=dev)
    steps = dict(
        cells=lambda: _abi.call(lib.hsr_nn_cells, "cells", dev, X, Y, Z, *g.origin, g.cell, n, pb.data_ptr(), cells.data_ptr()),
        sort=lambda: torch.sort(cells, stable=True),
        ranges=lambda: torch.searchsorted(sorted_cells, ids).to(torch.int32),
        pack=lambda: _abi.call(lib.hsr_nn_pack, "pack", dev, n, pb.data_ptr(), order.data_ptr(), packed.data_ptr()),
        constructor=lambda: mesh_eval.NearestGrid(pb, cell))
    steps["cells"]()
    sorted_cells, order = steps["sort"]()
    build = {name: [] for name in steps}
    for name, fn in steps.items():
        fn()
    for _ in range(a.reps):
        for name, fn in steps.items():
            build[name].append(event_ms(fn, 1 if name == "constructor" else a.batch)[0])
    occupied = int((g.cell_start[1:] > g.cell_start[:-1]).sum())
    report(what="build", dims=g.dims, cells=X * Y * Z, occupied_cells=occupied, points_per_occupied_cell=round(n / occupied, 2),
           ms={name: round(float(np.median(v)), 4) for name, v in build.items()}, reps=a.reps, batch=a.batch)

    # ---- the queries against the eager chains, alternating ----
    directions = {"a_to_b": (pa, "b", pb), "b_to_a": (pb, "a", pa)}
    times = {d: dict(grid=[], kernel=[], cdist=[], exact=[]) for d in directions}
    sorted_q, out_d2, out_index = {}, torch.empty(n, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    for d, (q, target, p) in directions.items():      # warm up every shape, and check the results at this size
        d2, index = grid[target].query(q)
        sorted_q[d] = q[torch.sort(grid[target]._cells(q), stable=True).indices].contiguous()      # what query() hands the kernel
        e_d2, e_index = eager_exact(q, p, a.chunk)
        c_d, c_index = eager_cdist(q, p, a.chunk)
        report(what="equal_" + d, d2_bits_equal=bool(torch.equal(d2.view(torch.int32), e_d2.view(torch.int32))),
               index_equal=bool(torch.equal(index.long(), e_index)), cdist_index_equal_share=float((c_index == index.long()).double().mean()),
               cdist_max_abs_diff_m=float((c_d - d2.sqrt()).abs().max()), mean_distance_m=float(d2.double().sqrt().mean()))
    for r in range(a.reps):
        for d, (q, target, p) in directions.items():
            t = grid[target]
            times[d]["grid"].append(event_ms(lambda: t.query(q), a.batch)[0])
            times[d]["kernel"].append(event_ms(lambda: _abi.call(lib.hsr_nn_query, "query", dev, *t.dims, *t.origin, t.cell, t.M, t.cell_start.data_ptr(),
                                                                t.packed.data_ptr(), n, sorted_q[d].data_ptr(), out_d2.data_ptr(),
                                                                out_index.data_ptr()), a.batch)[0])
            if r < a.eager_reps:
                times[d]["cdist"].append(event_ms(lambda: eager_cdist(q, p, a.chunk))[0])
                times[d]["exact"].append(event_ms(lambda: eager_exact(q, p, a.chunk))[0])
    for d in directions:
        t = {name: float(np.median(v)) for name, v in times[d].items() if v}
        report(what="query_" + d, samples=n, grid_ms=round(t["grid"], 4), kernel_only_ms=round(t["kernel"], 4), grid_ms_min_max=[round(min(times[d]["grid"]), 4), round(max(times[d]["grid"]), 4)],
               eager_cdist_ms=round(t["cdist"], 2), eager_exact_ms=round(t["exact"], 2), ratio_cdist=round(t["cdist"] / t["grid"], 1),
               ratio_exact=round(t["exact"] / t["grid"], 1), pairs=n * n, chunk=a.chunk, reps=a.reps, batch=a.batch, eager_reps=a.eager_reps)
    # the whole score as a user calls it
    rec = (vertices, faces, labels)
    mesh_eval.mesh_metrics(rec, rec, n_samples=n)
    ms_metrics, _ = event_ms(lambda: mesh_eval.mesh_metrics(rec, rec, n_samples=n))
    report(what="mesh_metrics", samples=n, ms=round(ms_metrics, 3))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
