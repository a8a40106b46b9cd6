#!/usr/bin/env python3
"""Measures the pictures of a mesh on the device (include/shade/hsr_mesh_shade.h; EXPERIMENTS.md §25): the reconstructed room of
tools/bench_mesh_depth.py (about a million faces), one 1200x680 view from its middle.
    normals          hsr_mesh_normals                      against  the same in eager torch: two gathers, a cross, three index_add_, a normalise
    shade_1          hsr_mesh_shade, the "shaded" picture  against  the eager composition of that picture from the same face image
    shade_5          hsr_mesh_shade, all five pictures     against  the eager composition of the five
    render_5         MeshRenderer.render: the depth launch and the five pictures
The eager compositions gather by the face image, form the barycentric weights, interpolate and normalise the normal, shade and convert
to uint8 — what a caller without the kernel would write; they are not bit-equal to the header's rule (torch fuses nothing and rounds
where it likes), so the largest byte difference against the kernel's pictures is printed with the times.  A call's time is device
events around warmed-up calls: the median, least and largest of --repeats windows, the cases taking turns; a window is as many
back-to-back calls as fill --window-ms of device time (at least --reps), so that a 40 microsecond launch is not timed over a
millisecond.  One JSON line per measurement.

    python tools/bench_mesh_view.py [--reps N] [--repeats N] [--window-ms MS]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

AMBIENT, ALBEDO, BACKGROUND = 0.25, (0.8, 0.8, 0.8), (255, 255, 255)


def eager_normals(v, f):
    import torch
    f = f.long()
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = torch.cross(b - a, c - a, dim=1)
    out = torch.zeros_like(v)
    for k in range(3):
        out.index_add_(0, f[:, k], n)
    return torch.nn.functional.normalize(out, dim=1)


def eager_pictures(v, f, normals, rgb, labels, scalar, face, w2c, k, H, W, names, label_table, scalar_table, scalar_range):
    """the pictures `names` in eager torch from the face image, by the header's formulas without its rounding order"""
    import torch
    dev = v.device
    m = torch.as_tensor(w2c, dtype=torch.float32, device=dev)
    hit = face >= 0
    tri = f.long()[face.clamp(min=0).long()]                       # [H,W,3]
    cam = v @ m[:3, :3].T + m[:3, 3]
    A, B, C = cam[tri[..., 0]], cam[tri[..., 1]], cam[tri[..., 2]]      # [H,W,3] each
    nA, nB, nC = torch.cross(B, C, dim=-1), torch.cross(C, A, dim=-1), torch.cross(A, B, dim=-1)
    det = (A * nA).sum(-1)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    ray = torch.stack([(xs - float(k[0][2])) / float(k[0][0]), (ys - float(k[1][2])) / float(k[1][1]), torch.ones_like(xs)], -1)
    w = torch.stack([(ray * nA).sum(-1), (ray * nB).sum(-1), (ray * nC).sum(-1)], -1)
    s = w.sum(-1, keepdim=True)
    bary = w / s
    p = ray * (det.unsqueeze(-1) / s)
    view = -torch.nn.functional.normalize(p, dim=-1)
    rot = normals @ m[:3, :3].T
    n = torch.nn.functional.normalize((bary.unsqueeze(-1) * rot[tri]).sum(-2), dim=-1)
    n = torch.where(((n * p).sum(-1, keepdim=True) > 0), -n, n)
    shade = AMBIENT + (1 - AMBIENT) * (n * view).sum(-1, keepdim=True).abs()
    bg = torch.tensor(BACKGROUND, dtype=torch.uint8, device=dev)

    def to_bytes(c):
        return torch.where(hit.unsqueeze(-1), (c.clamp(0, 1) * 255).round().to(torch.uint8), bg)

    out = {}
    for name in names:
        if name == "shaded":
            out[name] = to_bytes(torch.tensor(ALBEDO, device=dev) * shade)
        elif name == "colour":
            out[name] = to_bytes((bary.unsqueeze(-1) * rgb[tri].float()).sum(-2) / 255 * shade)
        elif name == "normals":
            out[name] = to_bytes(n * torch.tensor([0.5, -0.5, -0.5], device=dev) + 0.5)
        elif name == "labels":
            lab = labels[tri.gather(-1, bary.argmax(-1, keepdim=True)).squeeze(-1)].long()
            ok = (lab >= 0) & (lab < label_table.shape[0])
            col = label_table[lab.clamp(0, label_table.shape[0] - 1)].float() / 255 * shade
            out[name] = to_bytes(torch.where(ok.unsqueeze(-1), col, torch.zeros_like(col)))
        elif name == "scalar":
            t = (bary * scalar[tri]).sum(-1)
            idx = (((t - scalar_range[0]) / (scalar_range[1] - scalar_range[0])).clamp(0, 1) * 255).long()
            out[name] = to_bytes(scalar_table[idx].float() / 255 * shade)
    return out


def window(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30, help="calls per timed window, at least")
    ap.add_argument("--window-ms", type=float, default=100.0, help="device time a window should fill")
    ap.add_argument("--repeats", type=int, default=7, help="windows per case; the cases take turns")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_view.py needs a GPU")
    import bench_mesh as B
    from diff_gaussian_rasterization import _abi
    from hsr_utils import export, mesh, mesh_view
    dev = torch.device("cuda", torch.cuda.current_device())
    k = np.array([[B.FX, 0, B.W / 2 - 0.5], [0, B.FX, B.H / 2 - 0.5], [0, 0, 1]], np.float32)
    dims, h = (256, 256, 256), 0.02      # the room of bench_mesh_depth.py: twelve views fused into 256^3 points at 2 cm, then its surface
    origin = tuple(-h * (d - 1) / 2 for d in dims)
    room = mesh.TsdfVolume(origin, dims, h, labels=True)
    for p in [B.rotation(ax, ay) for ax in (-0.5, 0.0, 0.5) for ay in np.linspace(0, 2 * np.pi, 4, endpoint=False)]:
        depth, colour, labels = B.room_view(p, dev)
        room.integrate(depth, p, k, color=colour, labels=labels)
    v, f, rgb, lab = room.extract()
    del room
    lab = lab.to(torch.int32)
    view = B.rotation(0.2, 0.6)
    scalar = v.norm(dim=1)
    scalar_range = (0.5, 2.5)
    names = ("shaded", "colour", "normals", "labels", "scalar")
    label_table, scalar_table = export.label_colormap(256, dev), export.jet_colormap(dev)
    renderer = mesh_view.MeshRenderer(v, f, B.H, B.W, rgb=rgb, labels=lab)
    kw = dict(ambient=AMBIENT, albedo=ALBEDO, background=BACKGROUND, scalar=scalar, scalar_range=scalar_range)
    first = renderer.render(view, k, names, **kw)
    face = first["face"]
    common = dict(lib=os.path.basename(_abi.LIB_PATH), faces=int(f.shape[0]), vertices=int(v.shape[0]), image=[B.H, B.W],
                  covered=round(float((face >= 0).float().mean()), 4))

    # hsr_mesh_shade alone: the same face image every call, the job structs built once
    def shade_call(pictures):
        jobs = (_abi.hsr_shade_job * len(pictures))()
        outs = []
        for job, name in zip(jobs, pictures):
            job.kind, job.lit, job.ambient = mesh_view._KINDS[name], 1, AMBIENT
            job.normals = renderer.normals.data_ptr()
            job.albedo[:] = ALBEDO
            job.background[:] = list(BACKGROUND) + [0]
            if name == "colour":
                job.attr = rgb.data_ptr()
            elif name == "labels":
                job.attr, job.table, job.n = lab.data_ptr(), label_table.data_ptr(), 256
            elif name == "scalar":
                job.attr, job.table, job.n, job.lo, job.hi = scalar.data_ptr(), scalar_table.data_ptr(), 256, scalar_range[0], scalar_range[1]
            outs.append(torch.empty((B.H, B.W, 3), dtype=torch.uint8, device=dev))
            job.out = outs[-1].data_ptr()
        m = np.ascontiguousarray(view, dtype=np.float32)
        args = (v.shape[0], f.shape[0], v.data_ptr(), f.data_ptr(), B.H, B.W, float(k[0][0]), float(k[1][1]), float(k[0][2]), float(k[1][2]),
                m.ctypes.data_as(_abi.fp), face.data_ptr(), len(pictures), jobs)
        return (lambda: _abi.call(_abi.lib.hsr_mesh_shade, "hsr_mesh_shade", dev, *args)), (outs, m, jobs)

    shade_1, keep_1 = shade_call(("shaded",))
    shade_5, keep_5 = shade_call(names)
    eager = lambda pictures: eager_pictures(v, f, renderer.normals, rgb, lab, scalar, face, view, k, B.H, B.W, pictures, label_table,
                                            scalar_table, scalar_range)
    calls = {
        "normals": lambda: mesh_view.vertex_normals(v, f),
        "normals_eager": lambda: eager_normals(v, f),
        "shade_1": shade_1,
        "shade_1_eager": lambda: eager(("shaded",)),
        "shade_5": shade_5,
        "shade_5_eager": lambda: eager(names),
        "render_5": lambda: renderer.render(view, k, names, **kw),
    }
    # the eager pictures against the kernel's, and the eager normals against the kernel's
    got = eager(names)
    diff = {n: int((got[n].int() - first[n].int()).abs().max()) for n in names}
    off = {n: round(float(((got[n].int() - first[n].int()).abs() > 1).any(-1).float().mean()), 6) for n in names}
    cos = (eager_normals(v, f) * renderer.normals).sum(1)
    print(json.dumps(dict(what="eager_against_kernel", largest_byte_difference=diff, share_of_pixels_off_by_more_than_one=off,
                          least_cosine_of_normals=round(float(cos[cos != 0].min()), 6), **common)), flush=True)
    for n, fn in calls.items():      # warm up every shape
        fn()
        fn()
    torch.cuda.synchronize()
    reps = {n: max(a.reps, int(np.ceil(a.window_ms / max(window(fn, 5), 1e-3)))) for n, fn in calls.items()}
    times = {n: [] for n in calls}
    for _ in range(a.repeats):
        for n, fn in calls.items():
            times[n].append(window(fn, reps[n]))
    for n, ts in times.items():
        print(json.dumps(dict(what="mesh_view", case=n, ms=round(float(np.median(ts)), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4),
                              reps=reps[n], repeats=a.repeats, **common)), flush=True)
    del keep_1, keep_5


if __name__ == "__main__":
    main()
