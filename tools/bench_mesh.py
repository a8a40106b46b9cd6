#!/usr/bin/env python3
"""Measures the mesh path on the device (include/ext/hsr_tsdf.h; EXPERIMENTS.md §19): one 1200x680 view with colour and labels fused
into a 256^3 and a 512x512x256 volume by hsr_tsdf_integrate against the eager torch chain of the same arithmetic, the kernel's achieved
bytes per second against the bytes it must move, and the extraction of a fused synthetic room step by step (count / cumsum / faces /
unique / vertices).  Times are device events around warmed-up work; one JSON line per measurement.

    python tools/bench_mesh.py [--reps N] [--views N]

The scene is a box room seen from its middle: the depth of every pixel is the distance along the camera's axis to the first wall.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))

W, H, FX = 1200, 680, 600.0
ROOM = (2.0, 1.8, 1.0)      # half sizes in metres; the camera stands in the middle


def rotation(ax, ay):
    import numpy as np
    cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    m = np.eye(4, dtype=np.float32)
    m[:3, :3] = rx @ ry
    return m


def room_view(w2c, dev):
    """(depth [H,W], colour [3,H,W], labels int64 [H,W]) of the room from the pose w2c (a rotation about the room's middle)"""
    import torch
    k = (FX, FX, W / 2 - 0.5, H / 2 - 0.5)
    v, u = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    ray = torch.stack([(u - k[2]) / k[0], (v - k[3]) / k[1], torch.ones_like(u)])      # camera frame, z = 1
    world = torch.einsum("ji,jhw->ihw", torch.tensor(w2c[:3, :3], device=dev), ray)      # R^T ray
    half = torch.tensor(ROOM, device=dev).reshape(3, 1, 1)
    t = (half / world.abs().clamp_min(1e-12))
    depth, wall = t.min(dim=0)      # ray = (.., .., 1) in the camera frame: the parameter IS the depth along the axis
    hit = world * depth
    colour = (0.5 + 0.5 * torch.sin(3.0 * hit + wall.float())).contiguous()
    labels = (wall * 2 + (torch.gather(world, 0, wall[None])[0] > 0)).to(torch.int64)
    return depth.contiguous(), colour, labels


def eager_integrate(vol, grid_points, depth, colour, labels, w2c, k, trunc, max_weight):
    """the arithmetic of hsr_tsdf_integrate as eager torch operations on volume-sized tensors"""
    import torch
    px, py, pz = grid_points
    m = w2c
    xc = ((m[0][0] * px + m[0][1] * py) + m[0][2] * pz) + m[0][3]
    yc = ((m[1][0] * px + m[1][1] * py) + m[1][2] * pz) + m[1][3]
    zc = ((m[2][0] * px + m[2][1] * py) + m[2][2] * pz) + m[2][3]
    ok = zc > 0
    fu = torch.floor(k[0] * (xc / zc) + k[2] + 0.5)
    fv = torch.floor(k[1] * (yc / zc) + k[3] + 0.5)
    ok &= (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
    pix = torch.where(ok, fv, torch.zeros_like(fv)).long() * W + torch.where(ok, fu, torch.zeros_like(fu)).long()
    d = depth.reshape(-1)[pix]
    ok &= (d > 0) & torch.isfinite(d)
    sdf = d - zc
    ok &= ~(sdf < -trunc)
    t = torch.clamp_max(sdf / trunc, 1.0)
    w = vol["weight"]
    vol["tsdf"] = torch.where(ok, (vol["tsdf"] * w + t) / (w + 1), vol["tsdf"])
    vol["weight"] = torch.where(ok, torch.clamp_max(w + 1, max_weight), w)
    band = ok & (sdf.abs() <= trunc)
    cw = vol["cweight"]
    flat = colour.reshape(3, -1)
    vol["color"] = torch.stack([torch.where(band, (vol["color"][c] * cw + flat[c][pix]) / (cw + 1), vol["color"][c]) for c in range(3)])
    vol["cweight"] = torch.where(band, torch.clamp_max(cw + 1, max_weight), cw)
    closer = band & (sdf.abs() < vol["best"])
    vol["best"] = torch.where(closer, sdf.abs(), vol["best"])
    vol["label"] = torch.where(closer, labels.reshape(-1)[pix].int(), vol["label"])


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--views", type=int, default=12, help="views fused into the room before the extraction")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh.py needs a GPU")
    from hsr_utils import mesh
    dev = torch.device("cuda", torch.cuda.current_device())
    k = np.array([[FX, 0, W / 2 - 0.5], [0, FX, H / 2 - 0.5], [0, 0, 1]], np.float32)
    poses = [rotation(ax, ay) for ax in (-0.5, 0.0, 0.5) for ay in np.linspace(0, 2 * np.pi, max(1, a.views // 3), endpoint=False)]
    views = [room_view(p, dev) for p in poses]
    for dims, h in (((256, 256, 256), 0.02), ((512, 512, 256), 0.01)):
        origin = tuple(-h * (d - 1) / 2 for d in dims)
        N = dims[0] * dims[1] * dims[2]
        vol = mesh.TsdfVolume(origin, dims, h, labels=True)
        depth, colour, labels = views[0]
        vol.integrate(depth, poses[0], k, color=colour, labels=labels)
        n_hit, n_band = int((vol.weight > 0).sum()), int((vol.cweight > 0).sum())
        ms = timed(lambda: vol.integrate(depth, poses[0], k, color=colour, labels=labels), a.reps)
        # what one view must move: tsdf and weight read and written where a point is updated, cweight, three colour planes, best and
        # label read and written in the band, and one gathered depth (colour, label) per such point
        need = n_hit * (16 + 4) + n_band * (48 + 12 + 8)
        whole = N * 8 + n_hit * 8 + n_band * 96      # the same with every point's tsdf and weight read: a plain stream would move this
        print(json.dumps(dict(what="integrate", dims=dims, voxels=N, updated=n_hit, band=n_band, ms=round(ms, 4), bytes_needed=need,
                              GBps_needed=round(need / ms / 1e6, 1), GBps_if_streamed=round(whole / ms / 1e6, 1),
                              Gvoxels_per_s=round(N / ms / 1e6, 2))), flush=True)
        # the eager chain on the same state
        with torch.no_grad():
            lin = torch.arange(N, device=dev)
            i, j, kk = lin % dims[0], (lin // dims[0]) % dims[1], lin // (dims[0] * dims[1])
            pts = tuple(o + h * q.float() for o, q in zip(origin, (i, j, kk)))
            del lin, i, j, kk
            state = dict(tsdf=torch.ones(N, device=dev), weight=torch.zeros(N, device=dev), color=torch.zeros(3, N, device=dev),
                         cweight=torch.zeros(N, device=dev), best=torch.full((N,), float("inf"), device=dev),
                         label=torch.full((N,), -1, dtype=torch.int32, device=dev))
            kt = (float(k[0][0]), float(k[1][1]), float(k[0][2]), float(k[1][2]))
            run = lambda: eager_integrate(state, pts, depth, colour, labels, poses[0].tolist(), kt, vol.trunc, vol.max_weight)
            run()
            fresh = mesh.TsdfVolume(origin, dims, h, labels=True).integrate(depth, poses[0], k, color=colour, labels=labels)
            same = {n: bool(torch.equal(getattr(fresh, n).reshape(-1), state[n].reshape(-1))) for n in ("weight", "cweight", "label")}
            diff = float((fresh.tsdf.reshape(-1) - state["tsdf"]).abs().max())
            ms_eager = timed(run, max(3, a.reps // 10))
            peak = torch.cuda.max_memory_allocated() / 2 ** 30
        print(json.dumps(dict(what="integrate_eager_torch", dims=dims, ms=round(ms_eager, 3), ratio=round(ms_eager / ms, 1), equal=same,
                              tsdf_max_diff=diff, peak_GiB=round(peak, 2))), flush=True)
        del state, pts, fresh
        torch.cuda.empty_cache()
        if dims != (256, 256, 256):
            continue
        # the room: every view fused, then the extraction step by step
        room = mesh.TsdfVolume(origin, dims, h, labels=True)
        ms_all = timed(lambda: [room.integrate(d, p, k, color=c, labels=lab) for p, (d, c, lab) in zip(poses, views)], 3) / len(poses)
        X, Y, Z = dims
        from diff_gaussian_rasterization import _abi
        lib = _abi.lib
        counts = torch.empty(N, dtype=torch.int32, device=dev)
        t_count = timed(lambda: _abi.call(lib.hsr_tsdf_count, "count", dev, X, Y, Z, room.tsdf.data_ptr(), room.weight.data_ptr(), counts.data_ptr()), 10)
        t_cumsum = timed(lambda: torch.cumsum(counts, 0, dtype=torch.int64), 10)
        offsets = torch.cumsum(counts, 0, dtype=torch.int64)
        T = int(offsets[-1])
        keys = torch.empty((T, 3), dtype=torch.int64, device=dev)
        t_faces = timed(lambda: _abi.call(lib.hsr_tsdf_faces, "faces", dev, X, Y, Z, room.tsdf.data_ptr(), room.weight.data_ptr(), offsets.data_ptr(), T,
                                          keys.data_ptr()), 10)
        t_unique = timed(lambda: torch.unique(keys, return_inverse=True), 5)
        vkeys, _inv = torch.unique(keys, return_inverse=True)
        V = int(vkeys.numel())
        out = (torch.empty((V, 3), device=dev), torch.empty((V, 3), dtype=torch.uint8, device=dev), torch.empty(V, dtype=torch.int32, device=dev))
        t_vertices = timed(lambda: _abi.call(lib.hsr_tsdf_vertices, "vertices", dev, X, Y, Z, *origin, h, V, vkeys.data_ptr(), room.tsdf.data_ptr(),
                                             room.color.data_ptr(), room.cweight.data_ptr(), room.label.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                             out[2].data_ptr()), 10)
        t_extract = timed(room.extract, 3)
        print(json.dumps(dict(what="extract_room", dims=dims, views=len(poses), ms_per_view=round(ms_all, 4), faces=T, vertices=V,
                              ms=dict(count=round(t_count, 3), cumsum=round(t_cumsum, 3), faces=round(t_faces, 3), unique=round(t_unique, 3),
                                      vertices=round(t_vertices, 3), extract_call=round(t_extract, 3)))), flush=True)


if __name__ == "__main__":
    main()
