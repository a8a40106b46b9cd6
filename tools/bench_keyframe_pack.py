#!/usr/bin/env python3
"""Times the packed keyframe store (include/ext/hsr_keyframe_pack.h) on one keyframe of 1200x680 with L = 5 label planes and L = 0,
against what the same work costs in eager torch on the same tensors and the same device:

    hsr_keyframe_pack      one call (the pass and its one-workgroup finish), against the eager chain that does the same: multiply, clamp,
                           round, cast, divide back, compare the bit patterns and count, for colour, depth and labels;
    hsr_keyframe_unpack    one launch, against the eager widening: cast, divide, cast; labels to int64;
    one checkpoint         of a synthetic session of 50 such keyframes (L = 5): SlamSession.save_checkpoint (packed at save time)
                           against np.savez of the same keyframes as float32 / int64 planes, in seconds and bytes.

Device events around `--steps` calls after a warm-up; the wrapper's own work (allocation of the outputs, argument marshalling) is inside
both sides.  Outputs are compared before anything is timed.  One JSON line.

    python tools/bench_keyframe_pack.py [--steps 200] [--keyframes 50]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_keyframe_pack.py --keyframes 0      # kernel times, a run of its own
"""
import argparse
import json
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))

H, W, SCALE = 680, 1200, 6553.5


def keyframe(L, dev, seed=0):
    """planes as ingest() at sensor size leaves them: float(v) / 255 and float(double(q) / scale), labels below 2^16"""
    g = torch.Generator().manual_seed(seed)
    color = (torch.randint(0, 256, (3, H, W), generator=g).float().double() / 255.0).float()
    depth = (torch.randint(0, 65536, (1, H, W), generator=g).double() / SCALE).float()
    labels = torch.randint(0, 102, (L, H, W), generator=g) if L else None
    return color.to(dev), depth.to(dev), None if labels is None else labels.to(dev)


def eager_pack(color, depth, labels):
    """the codes and the three counts, in eager torch"""
    v = torch.round((color * 255.0).clamp(0, 255))
    bad_c = ((v.double() / 255.0).float().view(torch.int32) != color.view(torch.int32)).sum()
    q = torch.round((depth.double() * SCALE).clamp(0, 65535))
    bad_d = ((q / SCALE).float().view(torch.int32) != depth.view(torch.int32)).sum()
    out = [v.to(torch.uint8), q.to(torch.int32).to(torch.int16)]
    bad_l = torch.zeros((), dtype=torch.int64, device=color.device)
    if labels is not None:
        bad_l = ((labels < 0) | (labels > 65535)).sum()
        out.append(labels.clamp(0, 65535).to(torch.int32).to(torch.int16))
    return out, torch.stack((bad_c, bad_d, bad_l))


def eager_unpack(c8, d16, l16):
    color = (c8.float().double() / 255.0).float()
    depth = ((d16.to(torch.int32) & 0xffff).double() / SCALE).float()
    labels = None if l16 is None else (l16.to(torch.int64) & 0xffff)
    return color, depth, labels


def device_us(run, steps):
    for _ in range(10):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / steps, 2)


def measure_kernels(steps):
    from hsr_utils import checkpoint
    dev = torch.device("cuda:0")
    res = {}
    for L in (5, 0):
        color, depth, labels = keyframe(L, dev)
        pk = checkpoint.pack_keyframe(color, depth, labels, SCALE)
        codes = dict(pk.codes)
        want, counts = eager_pack(color, depth, labels)
        assert pk.lossy_counts == (0, 0, 0) and counts.tolist() == [0, 0, 0]
        assert torch.equal(codes["color"], want[0]) and torch.equal(codes["depth"], want[1].view(1, H, W)[0])
        assert L == 0 or torch.equal(codes["labels"], want[2])
        back, eager_back = checkpoint.unpack_keyframe(pk), eager_unpack(codes["color"], codes["depth"], codes.get("labels"))
        assert torch.equal(back[0], color) and torch.equal(back[1], depth) and torch.equal(eager_back[0], color)
        assert torch.equal(eager_back[1].view_as(depth), depth) and (L == 0 or (torch.equal(back[2], labels) and torch.equal(eager_back[2], labels)))
        n = H * W
        r = {"pack_us": device_us(lambda: checkpoint.pack_keyframe(color, depth, labels, SCALE), steps),
             "eager_pack_us": device_us(lambda: eager_pack(color, depth, labels), steps),
             "unpack_us": device_us(lambda: checkpoint.unpack_keyframe(pk), steps),
             "eager_unpack_us": device_us(lambda: eager_unpack(codes["color"], codes["depth"], codes.get("labels")), steps),
             "bytes_moved": n * (16 + 8 * L) + n * (5 + 2 * L)}      # the float / int64 planes once and the codes once, either way
        r["pack_GBps"] = round(r["bytes_moved"] / (r["pack_us"] * 1e-6) / 1e9, 1)
        r["unpack_GBps"] = round(r["bytes_moved"] / (r["unpack_us"] * 1e-6) / 1e9, 1)
        res["L%d" % L] = r
    return res


def measure_checkpoint(keyframes):
    """a session by hand: a small map, `keyframes` keyframes of the full size with 5 label planes"""
    from hsr_utils import slam
    dev = torch.device("cuda:0")
    lrs = dict(means3D=0.0, rgb_colors=0.0, unnorm_rotations=0.0, logit_opacities=0.0, log_scales=0.0, cam_unnorm_rots=0.0, cam_trans=0.0, semantic=0.0)
    head = dict(num_iters=1, lrs=lrs, loss_weights=dict(im=0.5, depth=1.0, sem=0.05), sil_thres=0.5)
    cfg = dict(map_every=1, keyframe_every=5, mapping_window_size=4, num_frames=5 * keyframes, tracking=head, mapping=head, num_semantic=[6, 10, 10, 10],
               png_depth_scale=SCALE)
    cam = types.SimpleNamespace(image_height=H, image_width=W, viewmatrix=torch.eye(4, device=dev)[None])
    s = slam.SlamSession(cfg, torch.eye(3, device=dev), torch.eye(4, device=dev), cam)
    P, frames = 1000, 5 * keyframes
    s.params = {k: torch.nn.Parameter(torch.rand(P, n, device=dev)) for k, n in (("means3D", 3), ("rgb_colors", 3), ("unnorm_rotations", 4),
                                                                                  ("logit_opacities", 1), ("log_scales", 1), ("semantic", 36))}
    s.params["cam_unnorm_rots"] = torch.nn.Parameter(torch.rand(1, 4, frames, device=dev))
    s.params["cam_trans"] = torch.nn.Parameter(torch.rand(1, 3, frames, device=dev))
    s.variables = {k: torch.zeros(P, device=dev) for k in ("max_2D_radius", "means2D_gradient_accum", "denom", "timestep")}
    s.variables["scene_radius"] = torch.tensor(1.0, device=dev)
    s.gt_w2c_all_frames = [torch.eye(4, device=dev) for _ in range(frames)]
    for i in range(keyframes):
        color, depth, labels = keyframe(5, dev, seed=i)
        s.keyframe_list.append({"id": 5 * i, "est_w2c": torch.eye(4, device=dev), "color": color, "depth": depth, "label_gt": labels, "cam": cam,
                                "intrinsics": s.intrinsics})
        s.keyframe_time_indices.append(5 * i)
    res = {"keyframes": keyframes}
    with tempfile.TemporaryDirectory() as tmp:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        paths = s.save_checkpoint(os.path.join(tmp, "packed"))
        res["packed_checkpoint_s"] = round(time.perf_counter() - t0, 3)
        res["packed_checkpoint_bytes"] = sum(os.path.getsize(p) for p in paths)
        t0 = time.perf_counter()
        raw = {}
        for i, kf in enumerate(s.keyframe_list):
            raw["kf%d.color" % i], raw["kf%d.depth" % i], raw["kf%d.labels" % i] = (kf[k].cpu().numpy() for k in ("color", "depth", "label_gt"))
        np.savez(os.path.join(tmp, "raw.npz"), **raw)
        res["raw_savez_s"] = round(time.perf_counter() - t0, 3)
        res["raw_savez_bytes"] = os.path.getsize(os.path.join(tmp, "raw.npz"))
        t0 = time.perf_counter()
        b = slam.SlamSession(cfg, torch.eye(3, device=dev), torch.eye(4, device=dev), cam, keyframe_store="packed")
        b.load_checkpoint(os.path.join(tmp, "packed"), frames - 1)
        torch.cuda.synchronize()
        res["packed_load_s"] = round(time.perf_counter() - t0, 3)
    res["bytes_ratio"] = round(res["raw_savez_bytes"] / res["packed_checkpoint_bytes"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--keyframes", type=int, default=50, help="keyframes of the synthetic session; 0 skips the checkpoint (a kernel trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_keyframe_pack.py needs a GPU")
    res = {"bench": "keyframe_pack", "H": H, "W": W, "depth_scale": SCALE, "steps": a.steps}
    res.update(measure_kernels(a.steps))
    if a.keyframes > 0:
        res["checkpoint"] = measure_checkpoint(a.keyframes)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
