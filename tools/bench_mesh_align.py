#!/usr/bin/env python3
"""Measures one pass of the mesh registration on the device (include/align/hsr_mesh_align.h; EXPERIMENTS.md §24): N surface samples
(default 200 000) of a displaced copy of the room that tools/bench_mesh.py meshes against N samples of the room itself, drawn with two
seeds, and the same source with a tenth of its points moved into the empty middle of the room, about a metre from any target.  The fused
pass is ONE hsr_icp_step on the source as icp hands it over (sorted once by cell).  The comparison is the eager composition a user could
write without it: the transform in torch, NearestGrid.query (its two sorts and two scatters, and a search with no distance cap), a mask
and seventeen reductions; its sums must agree with the fused ones.  Both at the cell icp defaults to (max_dist) and at mesh_metrics' cell
(twice the samples' spacing).  Then a whole icp of at most 30 passes, host reads included.  Times are device events around warmed-up
work, the two paths alternating within this one call; one JSON line per measurement, and all of them in --out.

    python tools/bench_mesh_align.py [--samples N] [--reps R] [--batch B] [--eager-reps R] [--eager-batch B] [--max-dist D] [--out JSON]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def displacement(middle, degrees=3.0, metres=0.03):
    """`degrees` about a skew axis through `middle` and `metres` along another skew direction: float64 [4,4]"""
    import numpy as np
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.radians(degrees)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(r) * K + (1 - np.cos(r)) * (K @ K)
    T[:3, 3] = middle - T[:3, :3] @ middle + np.array([2.0, -1.0, 2.0]) / 3.0 * metres
    return T


def eager_pass(grid, targets, source, transform, max_dist):
    """the pass without hsr_icp_step: float64 [17] on the device"""
    import numpy as np
    import torch
    from hsr_utils import mesh_align
    moved = mesh_align.transform_points(source, transform)
    d2, index = grid.query(moved)
    m2 = float(np.float32(max_dist) * np.float32(max_dist))
    has = (index >= 0) & (d2 <= m2)
    w = has.double()
    p, q = moved.double(), targets[index.clamp_min(0).long()].double()
    sums = [w.sum()]
    sums += [(p[:, a] * w).sum() for a in range(3)]
    sums += [(q[:, a] * w).sum() for a in range(3)]
    sums += [(p[:, a] * q[:, b] * w).sum() for a in range(3) for b in range(3)]
    sums.append(torch.where(has, d2.double(), torch.zeros_like(w)).sum())
    return torch.stack(sums)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=20, help="timed rounds, the two paths alternating")
    ap.add_argument("--batch", type=int, default=10, help="back-to-back calls of the fused pass inside one timed window")
    ap.add_argument("--eager-reps", type=int, default=5, help="of those rounds, how many also time the eager pass")
    ap.add_argument("--eager-batch", type=int, default=2, help="back-to-back calls of the eager pass inside one timed window")
    ap.add_argument("--max-dist", type=float, default=0.1)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_align.py needs a GPU")
    from bench_mesh_eval import event_ms, room_mesh
    from hsr_utils import mesh_align, mesh_eval
    dev = torch.device("cuda", torch.cuda.current_device())
    n, results = a.samples, []

    def report(**kw):
        results.append(kw)
        print(json.dumps(kw), flush=True)

    vertices, faces, _labels = room_mesh(a.views, dev)
    area = float(mesh_eval.face_areas(vertices, faces).double().sum())
    targets = mesh_eval.sample_mesh(vertices, faces, n, 1)[0]
    lo, hi = vertices.min(dim=0).values.cpu().numpy().astype(np.float64), vertices.max(dim=0).values.cpu().numpy().astype(np.float64)
    middle = 0.5 * (lo + hi)
    motion = displacement(middle)
    plain = mesh_align.transform_points(mesh_eval.sample_mesh(vertices, faces, n, 0)[0], motion)
    floaters = plain.clone()
    g = torch.Generator(device="cpu").manual_seed(3)
    moved_rows = torch.randperm(n, generator=g)[:n // 10].to(dev)
    floaters[moved_rows] = (torch.as_tensor(middle, dtype=torch.float32) + torch.rand((n // 10, 3), generator=g) * 0.5 - 0.25).to(dev)
    spacing = float(np.sqrt(area / n))
    report(what="room", vertices=int(vertices.shape[0]), faces=int(faces.shape[0]), area_m2=round(area, 3), samples=n, spacing_m=round(spacing, 5),
           max_dist_m=a.max_dist, displaced_by_m=[round(float(v), 4) for v in (mesh_align.transform_points(vertices, motion) - vertices).norm(dim=1).aminmax()])

    identity = np.eye(4)
    for cell_name, cell in (("max_dist", a.max_dist), ("two_spacings", 2.0 * spacing)):
        grid = mesh_eval.NearestGrid(targets, cell)
        occupied = int((grid.cell_start[1:] > grid.cell_start[:-1]).sum())
        for source_name, source in (("plain", plain), ("floaters", floaters)):
            ordered = source[torch.sort(grid._cells(source), stable=True).indices].contiguous()      # as icp hands it over
            fused = lambda: mesh_align.icp_step(grid, ordered, identity, a.max_dist)
            eager = lambda: eager_pass(grid, targets, source, identity, a.max_dist)
            fused_sums, eager_sums = fused().cpu().numpy(), eager().cpu().numpy()      # warm both up, and hold them against each other
            far = grid.query(source[moved_rows])[0].sqrt() if source_name == "floaters" else None
            times = dict(fused=[], eager=[])
            for r in range(a.reps):
                times["fused"].append(event_ms(fused, a.batch)[0])
                if r < a.eager_reps:
                    times["eager"].append(event_ms(eager, a.eager_batch)[0])
            t = {k: float(np.median(v)) for k, v in times.items()}
            report(what="pass", cell=cell_name, cell_m=round(grid.cell, 5), dims=grid.dims, points_per_occupied_cell=round(n / occupied, 2),
                   source=source_name, samples=n, correspondences=int(fused_sums[0]), counts_equal=bool(fused_sums[0] == eager_sums[0]),
                   sums_max_rel_diff=float(np.max(np.abs(fused_sums - eager_sums) / np.maximum(np.abs(eager_sums), 1e-300))),
                   floaters_nearest_target_m=None if far is None else [round(float(far.min()), 3), round(float(far.max()), 3)],
                   fused_ms=round(t["fused"], 4), eager_ms=round(t["eager"], 4), ratio=round(t["eager"] / t["fused"], 2),
                   fused_ms_min_max=[round(min(times["fused"]), 4), round(max(times["fused"]), 4)],
                   eager_ms_min_max=[round(min(times["eager"]), 4), round(max(times["eager"]), 4)], reps=a.reps, batch=a.batch, eager_reps=a.eager_reps, eager_batch=a.eager_batch)

    # ---- the whole loop as a user calls it: the grid given, the sort, every pass and its host read ----
    grid = mesh_eval.NearestGrid(targets, a.max_dist)
    for source_name, source in (("plain", plain), ("floaters", floaters)):
        mesh_align.icp(source, grid, max_dist=a.max_dist)      # warm up
        walls = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = mesh_align.icp(source, grid, max_dist=a.max_dist)
            torch.cuda.synchronize()
            walls.append(1e3 * (time.perf_counter() - t0))
        back = np.linalg.inv(motion)
        corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
        error = np.abs((corners @ got["transform"][:3, :3].T + got["transform"][:3, 3]) - (corners @ back[:3, :3].T + back[:3, 3])).max()
        report(what="icp", source=source_name, samples=n, passes=got["iterations"] + 1, updates=got["iterations"], converged=got["converged"],
               fitness=round(got["fitness"], 5), inlier_rmse_m=round(got["inlier_rmse"], 6), corner_error_m=round(float(error), 6),
               wall_ms=round(float(np.median(walls)), 3), wall_ms_min_max=[round(min(walls), 3), round(max(walls), 3)],
               ms_per_pass=round(float(np.median(walls)) / (got["iterations"] + 1), 4))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
