#!/usr/bin/env python3
"""Replays a finished run without a window: one picture per step of the map as it stood at that step, seen from the step's estimated
pose (hsr_utils.replay.replay_run; the reference's viz_scripts/online_recon*.py, and final_recon.py with --last).

    python tools/replay_run.py PARAMS_NPZ OUT_DIR [--every N] [--semantic] [--cloud] [--depth] [--last]

PARAMS_NPZ is the params.npz of a run (hsr_utils.map_io.save_params after finalize_params: it carries 'timestep', 'intrinsics',
'org_width' and 'org_height').  OUT_DIR receives {t}.png and, with --cloud, {t}.ply (x y z red green blue per pixel of the view).
--semantic renders through the semantic rasterizer; --depth writes jet-coloured depth pictures instead of colour.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("params_npz")
    ap.add_argument("out_dir")
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--semantic", action="store_true")
    ap.add_argument("--cloud", action="store_true")
    ap.add_argument("--depth", action="store_true")
    ap.add_argument("--last", action="store_true", help="the last step alone")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("replay_run.py needs a GPU")
    from hsr_utils import map_io, replay
    params = map_io.load_params(a.params_npz, device="cuda")
    steps = [int(params["cam_unnorm_rots"].shape[-1]) - 1] if a.last else None
    written = replay.replay_run(params, a.out_dir, every=a.every, semantic=a.semantic, picture="depth" if a.depth else "color", cloud=a.cloud,
                                steps=steps)
    print("wrote %d steps to %s" % (len(written), a.out_dir))


if __name__ == "__main__":
    main()
