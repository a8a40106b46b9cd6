#!/usr/bin/env python3
"""The mesh of a finished run: the finished map rendered from every N-th estimated pose, the rendered depth, colour and (with --semantic)
class labels fused into a truncated signed distance volume on the device, and the volume's surface written as a PLY file
(hsr_utils.mesh.mesh_run; include/ext/hsr_tsdf.h states the rules).

    python tools/mesh_run.py PARAMS_NPZ OUT_PLY [--voxel-size S] [--every N] [--semantic]
                             [--min-component-faces N] [--min-component-ratio R] [--largest-component]

PARAMS_NPZ is the params.npz of a run (hsr_utils.map_io.save_params after finalize_params: it carries 'intrinsics', 'w2c', 'org_width'
and 'org_height').  OUT_PLY receives vertex x y z red green blue (and label with --semantic) and triangular faces.  The volume is the
padded box of the map's Gaussians; a voxel size whose volume would not fit is refused with one that does.  With one of the component
options the small disconnected pieces of the surface are dropped on the device before the file is written (hsr_utils.mesh_clean;
include/surface/hsr_mesh_clean.h): components of fewer than N faces, of fewer than R times the largest one's faces, or all but the largest.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("params_npz")
    ap.add_argument("out_ply")
    ap.add_argument("--voxel-size", type=float, default=0.02, help="metres between sample points")
    ap.add_argument("--every", type=int, default=5)
    ap.add_argument("--semantic", action="store_true", help="render through the semantic rasterizer and fuse the argmax class of every pixel")
    ap.add_argument("--sil-thres", type=float, default=0.5)
    ap.add_argument("--depth-max", type=float, default=0.0, help="ignore rendered depth beyond this (0: no limit)")
    ap.add_argument("--min-component-faces", type=int, default=0, help="drop connected components of fewer faces than this")
    ap.add_argument("--min-component-ratio", type=float, default=0.0, help="drop components of fewer faces than this part of the largest one's")
    ap.add_argument("--largest-component", action="store_true", help="keep the connected component of the most faces only")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mesh_run.py needs a GPU")
    from hsr_utils import map_io, mesh
    params = map_io.load_params(a.params_npz, device="cuda")
    path, nv, nf = mesh.mesh_run(params, a.out_ply, voxel_size=a.voxel_size, every=a.every, semantic=a.semantic, sil_thres=a.sil_thres,
                                 depth_max=a.depth_max, min_component_faces=a.min_component_faces,
                                 min_component_ratio=a.min_component_ratio, largest_component=a.largest_component)
    print("wrote %d vertices and %d faces to %s" % (nv, nf, path))


if __name__ == "__main__":
    main()
