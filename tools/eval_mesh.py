#!/usr/bin/env python3
"""Scores the mesh of a finished run against the ground-truth mesh of its scene, on the device (hsr_utils.mesh_eval.evaluate_mesh_run;
include/eval/hsr_mesh_eval.h states the rules): the run is meshed as tools/mesh_run.py meshes it, the ground truth is culled to the
vertices the estimated poses saw, both surfaces are sampled, and every sample's exact nearest neighbour on the other side gives accuracy,
completion, their ratios at the threshold, the F-score and, with --semantic, the 3D mIoU of the labels transferred by nearest neighbour.

    python tools/eval_mesh.py PARAMS_NPZ GT_PLY [--voxel-size S] [--every N] [--threshold T] [--semantic] [--out JSON]
                              [--depth-views N [--depth-seed S] [--depth-size H W]]
                              [--min-component-faces N] [--min-component-ratio R] [--largest-component]
                              [--align {icp,trajectory} [--align-max-dist D] [--align-iterations N] [--gt-poses NPY]]

PARAMS_NPZ is the params.npz of a run (hsr_utils.map_io.save_params after finalize_params).  GT_PLY is a mesh in the layout
hsr_utils.mesh.save_mesh_ply writes (vertex x y z [red green blue] [label], triangular faces), in the run's world frame.  One JSON
object on stdout, and in --out when given; distances are in metres.  With --depth-views N both meshes are also rendered to depth from N
views the sensor never took (hsr_utils.mesh_depth; include/recon/hsr_mesh_depth.h) and depth_l1, depth_l1_covered, depth_gt_cover,
depth_rec_cover and depth_views join the object; without it the object is what it was.  The component options are those of
tools/mesh_run.py: the run's mesh loses its small disconnected pieces before it is scored (hsr_utils.mesh_clean).  With --align the
run's mesh is registered to the (culled) ground truth before anything is scored (hsr_utils.mesh_align; include/align/hsr_mesh_align.h):
icp is rigid point-to-point ICP of surface samples from the identity, with a correspondence distance of --align-max-dist metres and at
most --align-iterations updates; trajectory applies the rigid map between the camera centres of the estimated poses and those of
--gt-poses, a .npy of [T,4,4] world-to-camera matrices.  align, align_transform and, for icp, align_fitness, align_rmse and
align_iterations join the object; without --align the object is what it was.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("params_npz")
    ap.add_argument("gt_ply")
    ap.add_argument("--voxel-size", type=float, default=0.02, help="metres between the sample points of the run's mesh")
    ap.add_argument("--every", type=int, default=5, help="every N-th estimated pose is meshed and culls the ground truth")
    ap.add_argument("--threshold", type=float, default=0.05, help="metres: the ratios' distance and the culling's depth slack")
    ap.add_argument("--samples", type=int, default=200000, help="points drawn on each surface")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--semantic", action="store_true", help="mesh through the semantic rasterizer and score the labels too")
    ap.add_argument("--classes", type=int, default=None, help="number of classes (default: one more than the largest label)")
    ap.add_argument("--no-cull", action="store_true", help="score against the whole ground-truth mesh")
    ap.add_argument("--sil-thres", type=float, default=0.5)
    ap.add_argument("--depth-views", type=int, default=0, help="also report Depth L1 of the two meshes from N virtual views")
    ap.add_argument("--depth-seed", type=int, default=0)
    ap.add_argument("--depth-size", type=int, nargs=2, default=None, metavar=("H", "W"), help="size of the depth images (default: the run's)")
    ap.add_argument("--out", default=None, help="also write the JSON object here")
    ap.add_argument("--min-component-faces", type=int, default=0, help="drop connected components of fewer faces than this")
    ap.add_argument("--min-component-ratio", type=float, default=0.0, help="drop components of fewer faces than this part of the largest one's")
    ap.add_argument("--largest-component", action="store_true", help="keep the connected component of the most faces only")
    ap.add_argument("--align", choices=("icp", "trajectory"), default=None, help="register the run's mesh to the ground truth before scoring")
    ap.add_argument("--align-max-dist", type=float, default=0.1, help="metres: the correspondence distance of --align icp")
    ap.add_argument("--align-iterations", type=int, default=30, help="the most updates --align icp makes")
    ap.add_argument("--gt-poses", default=None, metavar="NPY", help="[T,4,4] ground-truth world-to-camera matrices, for --align trajectory")
    a = ap.parse_args()
    if a.align == "trajectory" and a.gt_poses is None:
        ap.error("--align trajectory needs --gt-poses")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("eval_mesh.py needs a GPU")
    from hsr_utils import map_io, mesh_eval
    params = map_io.load_params(a.params_npz, device="cuda")
    extra = {}
    if a.align is not None:
        import numpy as np
        extra.update(align=a.align, align_max_dist=a.align_max_dist, align_iterations=a.align_iterations,
                     gt_w2cs=None if a.gt_poses is None else np.load(a.gt_poses))
    got = mesh_eval.evaluate_mesh_run(params, a.gt_ply, voxel_size=a.voxel_size, every=a.every, threshold=a.threshold, n_samples=a.samples,
                                      seed=a.seed, semantic=a.semantic, num_classes=a.classes, sil_thres=a.sil_thres, cull=not a.no_cull, depth_views=a.depth_views,
                                      depth_seed=a.depth_seed, depth_size=a.depth_size, min_component_faces=a.min_component_faces,
                                      min_component_ratio=a.min_component_ratio, largest_component=a.largest_component, **extra)
    result = {k: (v.tolist() if isinstance(v, torch.Tensor) else v) for k, v in got.items()}
    result.update(threshold=a.threshold, samples=a.samples, voxel_size=a.voxel_size, every=a.every)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
