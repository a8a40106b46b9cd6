#!/usr/bin/env python3
"""Times the per-frame map evaluation (include/hsr_eval.h, hsr_utils/evaluate.py evaluate_frame) at 1200x680, K=26, tree and leaf
modes (C=102 leaf classes), against an eager torch restatement of the reference's per-frame body on the same device (its per-class
loop with the host synchronisations and device->host copies it makes; the erosion as max_pool2d, since cv2 is absent) and the numpy
restatement of tests/eval_ref.py on the host.  One JSON line.

    python tools/bench_eval.py [--frames 50] [--torch-frames 3] [--no-cpu] [--trace OUTDIR]

--trace OUTDIR adds a per-kernel breakdown: a fresh child process runs the GPU part under `rocprofv3 --kernel-trace --stats`, in a run of
its own, writing under OUTDIR.  Numbers not taken are reported as "not measured"."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W, K = 680, 1200, 26
SIZES = [2, 4, 6, 6, 8, 102]
C_LEAF = SIZES[-1]


def inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    mapping = {str(leaf): tuple(int(rng.integers(0, s)) for s in SIZES[:-1]) for leaf in range(C_LEAF)}
    gt_im = torch.rand(3, H, W, generator=g)
    im = (gt_im + 0.05 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    gt_d = torch.rand(1, H, W, generator=g) * 5 + 0.5
    gt_d[:, :20] = 0
    d = gt_d + 0.05 * torch.randn(1, H, W, generator=g)
    opac = torch.rand(1, H, W, generator=g)
    # smooth logits: label regions the size a rendered map has, so that the boundary work is representative
    sem = F.interpolate(torch.randn(1, K, H // 20, W // 20, generator=g) * 3, size=(H, W), mode="bilinear", align_corners=False)[0]
    gt_lab = torch.randint(0, C_LEAF, (H // 40, W // 40), generator=g).repeat_interleave(40, 0).repeat_interleave(40, 1)
    gt_lab = F.pad(gt_lab, (0, W - gt_lab.shape[1], 0, H - gt_lab.shape[0]), value=0)
    return mapping, dict(im=im, gt_im=gt_im, depth=d, gt_depth=gt_d, final_opacity=opac, sem=sem, gt_lab=gt_lab)


def torch_reference_frame(dev, t, mode, mapping, mlp):
    """The reference's per-frame body in eager torch (utils/eval_helpers.py:1258-1498) minus MS-SSIM / LPIPS / plots: masks, PSNR and
    depth terms, labels (per-level softmax + argmax and one masked assignment per dict entry, or the 1x1 conv), then the per-class loop
    with its two .sum() checks, two device->host copies and two boundary erosions of d iterations (max_pool2d in place of cv2.erode)."""
    im, gt_im, depth, gt_d, opac, sem, gt_lab = (t[n] for n in ("im", "gt_im", "depth", "gt_depth", "final_opacity", "sem", "gt_lab"))
    valid = gt_d > 0
    rastered = depth * valid
    pres = opac.squeeze(0) > 0.5
    w_im, w_gt = im * pres * valid, gt_im * pres * valid
    mse = ((w_im - w_gt) ** 2).view(3, -1).mean(1, keepdim=True)
    psnr = (20 * torch.log10(1.0 / torch.sqrt(mse))).mean()
    diff = (rastered - gt_d) * pres
    rmse = (torch.sqrt(diff ** 2) * valid).sum() / valid.sum()
    l1 = (torch.abs(diff) * valid).sum() / valid.sum()
    out = [psnr.cpu().numpy(), l1.cpu().numpy(), rmse.cpu().numpy()]
    if mode == "tree":
        levels, b = [], 0
        for n in SIZES[:-1]:
            levels.append(torch.argmax(torch.softmax(sem[b:b + n].permute(1, 2, 0), dim=-1), dim=-1))
            b += n
        tl = torch.stack(levels)
        lab = torch.full((H, W), -1, dtype=torch.int64, device=dev)
        for key, value in mapping.items():
            idx = torch.all(tl == torch.tensor(value, device=dev).view(-1, 1, 1), dim=0)
            lab[idx] = int(key)
    else:
        lab = torch.argmax(F.softmax(mlp(sem.unsqueeze(0)).squeeze(0), dim=0), dim=0)
    d = max(1, int(round(0.02 * np.sqrt(H ** 2 + W ** 2))))

    def boundary(m):
        x = F.pad(m.view(1, 1, H, W), (1, 1, 1, 1), value=0.0)
        for _ in range(d):
            x = -F.max_pool2d(-x, 3, stride=1, padding=1)     # 3x3 erosion; the -inf padding of max_pool2d does not erode
        return m - x[0, 0, 1:-1, 1:-1]

    ious, bious = [], []
    for c in range(C_LEAF):
        pm, gm = (lab == c).float(), (gt_lab == c).float()
        if pm.sum() == 0 and gm.sum() == 0:                    # two host synchronisations
            continue
        pb, gb = boundary(pm), boundary(gm)
        pm_h, gm_h = pm.cpu().numpy(), gm.cpu().numpy()       # the reference's two device->host copies
        ious.append(np.logical_and(gm_h > 0, pm_h > 0).sum() / np.logical_or(gm_h > 0, pm_h > 0).sum())
        pb_h, gb_h = pb.cpu().numpy(), gb.cpu().numpy()
        bious.append(((gb_h * pb_h) > 0).sum() / ((gb_h + pb_h) > 0).sum())
    return out + [np.mean(ious), np.mean(bious)]


def measure_gpu(frames, torch_frames):
    from hsr_utils import evaluate as E
    dev = torch.device("cuda:0")
    mapping, host = inputs()
    t = {n: v.to(dev) for n, v in host.items()}
    table = E.tree_lookup_table(mapping, SIZES, device=dev)
    torch.manual_seed(1)
    mlp = torch.nn.Conv2d(K, C_LEAF, kernel_size=1).to(dev)
    res = {}
    for mode in ("tree", "leaf"):
        run = lambda: E.evaluate_frame(t["im"], t["gt_im"], t["depth"], t["gt_depth"], t["sem"], t["gt_lab"], mode,
                                       final_opacity=t["final_opacity"], sil_thres=0.5, level_sizes=SIZES, tree_table=table, mlp=mlp,
                                       num_classes=C_LEAF)
        for _ in range(5):
            out = run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        outs = [run() for _ in range(frames)]
        e1.record()
        torch.cuda.synchronize()
        res[mode + "_evaluate_frame_us"] = round(e0.elapsed_time(e1) * 1e3 / frames, 1)
        res[mode + "_scores"] = {k: float(v) for k, v in outs[-1].items()}
        if torch_frames > 0:
            with torch.no_grad():
                torch_reference_frame(dev, t, mode, mapping, mlp)     # warm-up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(torch_frames):
                    ref = torch_reference_frame(dev, t, mode, mapping, mlp)
                torch.cuda.synchronize()
            res[mode + "_torch_eager_ms"] = round((time.perf_counter() - t0) * 1e3 / torch_frames, 2)
            res[mode + "_torch_eager_scores"] = [float(x) for x in ref]
        else:
            res[mode + "_torch_eager_ms"] = "not measured"
    return res


def measure_cpu():
    import eval_ref as R
    mapping, host = inputs()
    h = {n: v.numpy() for n, v in host.items()}
    t0 = time.perf_counter()
    m = R.frame_metrics(h["im"], h["gt_im"], h["depth"], h["gt_depth"], h["final_opacity"], 0.5)
    lab = R.tree_to_leaf(R.tree_level_labels(h["sem"], SIZES), mapping)
    s = R.frame_miou(R.iou_counts(lab, h["gt_lab"], list(range(C_LEAF))))
    return {"tree_numpy_host_ms": round((time.perf_counter() - t0) * 1e3, 1), "tree_numpy_scores": [float(x) for x in list(m) + list(s)]}


def kernel_breakdown(outdir, frames):
    if shutil.which("rocprofv3") is None:
        return "not measured (no rocprofv3)"
    os.makedirs(outdir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--", sys.executable, os.path.abspath(__file__),
           "--gpu-only", "--frames", str(frames), "--torch-frames", "0"]
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    if r.returncode != 0:
        return "not measured (rocprofv3 exit %d)" % r.returncode
    files = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return "not measured (no kernel_stats.csv)"
    rows = []
    for row in csv.DictReader(open(files[0])):
        short = row["Name"].replace("(anonymous namespace)::", "").split("(")[0]
        if short:
            rows.append({"kernel": short[:60], "calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2)})
    rows.sort(key=lambda r: -r["avg_us"] * r["calls"])
    return rows[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--torch-frames", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--gpu-only", action="store_true", help="the profiled child: GPU part only, no JSON")
    ap.add_argument("--trace", default=None, help="directory for the rocprofv3 run")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py needs a GPU")
    if a.gpu_only:
        measure_gpu(a.frames, a.torch_frames)
        return
    res = {"bench": "eval_frame", "H": H, "W": W, "K": K, "leaf_classes": C_LEAF, "frames": a.frames}
    res.update(measure_gpu(a.frames, a.torch_frames))
    res.update(measure_cpu() if not a.no_cpu else {"tree_numpy_host_ms": "not measured"})
    res["kernels"] = kernel_breakdown(a.trace, 20) if a.trace else "not measured"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
