#!/usr/bin/env python3
"""Pictures of a mesh without a window: a PLY of tools/mesh_run.py (or any PLY hsr_utils.mesh.save_mesh_ply wrote) rendered on the
device from the estimated poses of its run, from an orbit round it, or both, and written as PNG files (hsr_utils.mesh_view;
include/shade/hsr_mesh_shade.h states the rule of every byte).

    python tools/render_mesh.py MESH_PLY OUT_DIR [--params PARAMS_NPZ --every N] [--orbit N] [--pictures shaded,colour,labels,normals,scalar]
                                [--gt GT_PLY] [--flat] [--size WxH] [--unlit] [--ambient A] [--elevation DEG]

With --params the views are every N-th estimated pose of the run (the views the mesh was fused from) at the run's own camera; --orbit
adds that many views on a circle round the mesh's bounds.  Without --params the views are the orbit alone (--orbit defaults to 8) and
the camera is a pinhole of 60 degrees across at --size (default 1200x680).  OUT_DIR receives {picture}_{i:04d}.png.  --gt: the
ground-truth mesh in the same frame; its gt_shaded_{i:04d}.png from the same views and, for the "scalar" picture, the heat map of the
mesh's distance to it.  "colour" and "labels" need a mesh with colours and labels.  --flat shades every face with its own normal.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mesh_ply")
    ap.add_argument("out_dir")
    ap.add_argument("--params", default=None, help="params.npz of the run: render from its estimated poses with its camera")
    ap.add_argument("--every", type=int, default=50, help="with --params: every N-th pose")
    ap.add_argument("--orbit", type=int, default=None, help="views on a circle round the mesh (default 0 with --params, else 8)")
    ap.add_argument("--pictures", default="shaded", help="comma-separated: shaded,colour,labels,normals,scalar")
    ap.add_argument("--gt", default=None, help="ground-truth PLY in the same frame")
    ap.add_argument("--flat", action="store_true", help="flat shading instead of smooth vertex normals")
    ap.add_argument("--size", default=None, help="WxH of the pictures")
    ap.add_argument("--unlit", action="store_true", help="colour, labels and scalar pictures without the shade")
    ap.add_argument("--ambient", type=float, default=0.25)
    ap.add_argument("--elevation", type=float, default=30.0, help="degrees of the orbit above the mesh's middle")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("render_mesh.py needs a GPU")
    from hsr_utils import map_io, mesh, mesh_view
    pictures = tuple(p for p in a.pictures.split(",") if p)
    size = None
    if a.size is not None:
        size = tuple(int(s) for s in a.size.lower().split("x"))
        if len(size) != 2:
            raise SystemExit("--size takes WxH")
    dev = torch.device("cuda", torch.cuda.current_device())
    parts = tuple(None if p is None else torch.as_tensor(np.ascontiguousarray(p), device=dev) for p in mesh.load_mesh_ply(a.mesh_ply))
    gt = None
    if a.gt is not None:
        gt = tuple(torch.as_tensor(np.ascontiguousarray(p), device=dev) for p in mesh.load_mesh_ply(a.gt)[:2])
    kw = dict(pictures=pictures, gt=gt, normals="flat" if a.flat else "smooth", lit=not a.unlit, ambient=a.ambient)
    if a.params is not None:
        params = map_io.load_params(a.params, device="cuda")
        paths = mesh_view.render_mesh_run(params, parts, a.out_dir, every=a.every, orbit=a.orbit or 0, size=size, elevation_deg=a.elevation, **kw)
    else:
        w, h = size or (1200, 680)
        fx = 0.5 * w / np.tan(np.deg2rad(30.0))
        k = np.array([[fx, 0, w / 2 - 0.5], [0, fx, h / 2 - 0.5], [0, 0, 1]])
        v = parts[0][torch.isfinite(parts[0]).all(dim=1)]
        views = mesh_view.orbit_views(v.min(dim=0).values, v.max(dim=0).values, 8 if a.orbit is None else a.orbit, elevation_deg=a.elevation)
        paths = mesh_view.render_mesh_views(parts, views, k, h, w, out_dir=a.out_dir, **kw)
    print("wrote %d pictures to %s" % (len(paths), a.out_dir))


if __name__ == "__main__":
    main()
