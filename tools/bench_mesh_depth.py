#!/usr/bin/env python3
"""Measures the depth image of a mesh on the device (include/recon/hsr_mesh_depth.h; EXPERIMENTS.md §21): one 1200x680 view, from the
middle of the room, of
    (a) the reconstructed room of tools/bench_mesh.py: about a million faces of a pixel or so;
    (b) the same plus a box of 12 faces around it, so that large faces occur as in a ground-truth mesh;
    (c) the 12 faces alone;
and Depth L1 of (a) against (b) per view (hsr_utils.mesh_depth.mesh_depth_l1, its one host read included).  A call's time is device
events around warmed-up calls, as the median, least and largest of --repeats windows of --reps calls, the cases taking turns; the time
per stage (the key image's fill, setup with the small faces, the sweep of the large ones, resolve) is the device time of each kernel from
torch.profiler in a pass of its own.  One JSON line per measurement.  (b) must cost no more than (a) plus (c) plus the spread between
repeats: a wall-sized face that sat on one lane would show here.

    python tools/bench_mesh_depth.py [--reps N] [--repeats N] [--views N] [--no-stages]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

BOX = (2.3, 2.1, 1.3)      # half sizes of the box around the room of bench_mesh.py (2.0, 1.8, 1.0)
STAGES = (("fill", ("fill", "memset")), ("setup_small", ("setup_kernel",)), ("sweep_large", ("sweep_kernel",)), ("resolve", ("resolve_kernel",)))


def box_mesh(half, dev):
    import torch
    hx, hy, hz = half
    v = torch.tensor([[-hx, -hy, -hz], [hx, -hy, -hz], [hx, hy, -hz], [-hx, hy, -hz], [-hx, -hy, hz], [hx, -hy, hz], [hx, hy, hz], [-hx, hy, hz]],
                     dtype=torch.float32, device=dev)
    quads = [(0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (3, 2, 6, 7), (0, 3, 7, 4), (1, 2, 6, 5)]
    f = torch.tensor([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=torch.int32, device=dev)
    return v, f


def window(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def stage_times(fn, reps):
    """device milliseconds per call of every stage, from the kernels' own durations; None with the reason when the profiler sees no kernel"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        events = [(e.key, float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))) for e in prof.key_averages()]
    except Exception as err:      # a profiler that is not there is no measurement: say so in the line
        return None, repr(err)
    out = {}
    for stage, words in STAGES:
        out[stage] = round(sum(us for key, us in events if any(w in key.lower() for w in words)) / reps / 1000.0, 4)
    if out["setup_small"] == 0 and out["resolve"] == 0:
        return None, "the profiler recorded no kernel of hsr_mesh_depth: %s" % sorted(k for k, _ in events)[:8]
    return out, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50, help="calls per timed window")
    ap.add_argument("--repeats", type=int, default=7, help="windows per case; the cases take turns")
    ap.add_argument("--views", type=int, default=8, help="views of the Depth L1 measurement")
    ap.add_argument("--no-stages", action="store_true", help="skip the profiler's pass")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_depth.py needs a GPU")
    import bench_mesh as B
    from diff_gaussian_rasterization import _abi
    from hsr_utils import mesh, mesh_depth
    dev = torch.device("cuda", torch.cuda.current_device())
    k = np.array([[B.FX, 0, B.W / 2 - 0.5], [0, B.FX, B.H / 2 - 0.5], [0, 0, 1]], np.float32)
    # the room of bench_mesh.py: twelve views fused into 256^3 points at 2 cm, then its surface
    dims, h = (256, 256, 256), 0.02
    origin = tuple(-h * (d - 1) / 2 for d in dims)
    room = mesh.TsdfVolume(origin, dims, h, labels=True)
    poses = [B.rotation(ax, ay) for ax in (-0.5, 0.0, 0.5) for ay in np.linspace(0, 2 * np.pi, 4, endpoint=False)]
    for p in poses:
        depth, colour, labels = B.room_view(p, dev)
        room.integrate(depth, p, k, color=colour, labels=labels)
    rv, rf, _rgb, _lab = room.extract()
    del room
    bv, bf = box_mesh(BOX, dev)
    meshes = {"a_room": (rv, rf), "b_room_and_box": (torch.cat([rv, bv]), torch.cat([rf, bf + rv.shape[0]])), "c_box": (bv, bf)}
    view = B.rotation(0.2, 0.6)
    renderers = {n: mesh_depth.MeshDepthRenderer(v, f, B.H, B.W) for n, (v, f) in meshes.items()}
    calls = {n: (lambda r=r: r.render(view, k)) for n, r in renderers.items()}
    common = dict(lib=os.path.basename(_abi.LIB_PATH), small_box=mesh_depth.SMALL_BOX, image=[B.H, B.W])
    print(json.dumps(dict(what="meshes", faces={n: int(f.shape[0]) for n, (_v, f) in meshes.items()}, **common)), flush=True)
    for n, fn in calls.items():      # warm up every shape; one call's time first, so that a case far off its expected cost shows at once
        fn()
        torch.cuda.synchronize()
        print(json.dumps(dict(what="first_call_after_warmup", case=n, faces=int(meshes[n][1].shape[0]), ms=round(window(fn, 1), 3))), flush=True)
        fn()
    torch.cuda.synchronize()
    times = {n: [] for n in calls}
    for _ in range(a.repeats):
        for n, fn in calls.items():
            times[n].append(window(fn, a.reps))
    med = {}
    for n, ts in times.items():
        d, f = calls[n]()
        med[n] = float(np.median(ts))
        print(json.dumps(dict(what="mesh_depth", case=n, faces=int(meshes[n][1].shape[0]), vertices=int(meshes[n][0].shape[0]),
                              covered=round(float((f >= 0).float().mean()), 4), ms=round(med[n], 4), ms_min=round(min(ts), 4),
                              ms_max=round(max(ts), 4), **common)), flush=True)
    spread = max(max(ts) - min(ts) for ts in times.values())
    print(json.dumps(dict(what="large_faces_do_not_serialise", b_ms=round(med["b_room_and_box"], 4),
                          a_plus_c_ms=round(med["a_room"] + med["c_box"], 4), spread_ms=round(spread, 4),
                          holds=bool(med["b_room_and_box"] <= med["a_room"] + med["c_box"] + spread), **common)), flush=True)
    # Depth L1 of the room against the room in its box, from views at the room's middle
    views = np.stack([B.rotation(ax, ay) for ax in (-0.3, 0.3) for ay in np.linspace(0, 2 * np.pi, max(1, a.views // 2), endpoint=False)])
    run = lambda: mesh_depth.mesh_depth_l1(meshes["a_room"], meshes["b_room_and_box"], views, k, B.H, B.W)
    got = run()
    per_view = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()      # ends in its host read
        per_view.append((time.perf_counter() - t0) * 1000.0 / len(views))
    print(json.dumps(dict(what="mesh_depth_l1", views=len(views), ms_per_view=round(float(np.median(per_view)), 4), ms_per_view_min=round(min(per_view), 4),
                          ms_per_view_max=round(max(per_view), 4), depth_l1=got["depth_l1"], depth_l1_covered=got["depth_l1_covered"],
                          gt_cover=got["gt_cover"], rec_cover=got["rec_cover"], **common)), flush=True)
    if a.no_stages:
        return
    for n, fn in calls.items():      # the profiler's pass, after every end-to-end number: tracing slows the host
        stages, why = stage_times(fn, max(5, a.reps // 5))
        print(json.dumps(dict(what="mesh_depth_stages", case=n, stage_ms=stages, note=why, **common)), flush=True)


if __name__ == "__main__":
    main()
