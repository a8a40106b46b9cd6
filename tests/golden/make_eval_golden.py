"""Generates tests/golden/eval/psnr_depth.npz: inputs and outputs of the reference's per-frame PSNR and depth terms, with its own
calc_psnr (utils/slam_external.py:49-51) imported from /root/reference in the build container and the mask / depth lines of
eval_semantic_tree_newrender (utils/eval_helpers.py:1258-1295) applied in torch fp32 as written there.  Only data is stored.
Run: python tests/golden/make_eval_golden.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
from utils.slam_external import calc_psnr  # noqa: E402


def reference_terms(im, gt_im, depth, gt_depth, final_opacity, sil_thres, use_sil):
    valid_depth_mask = gt_depth > 0
    rastered_depth = depth * valid_depth_mask
    presence_sil_mask = final_opacity.squeeze(0) > sil_thres
    if use_sil:
        weighted_im = im * presence_sil_mask * valid_depth_mask
        weighted_gt_im = gt_im * presence_sil_mask * valid_depth_mask
    else:
        weighted_im = im * valid_depth_mask
        weighted_gt_im = gt_im * valid_depth_mask
    psnr = calc_psnr(weighted_im, weighted_gt_im).mean()
    if use_sil:
        diff_depth_rmse = torch.sqrt((((rastered_depth - gt_depth) * presence_sil_mask) ** 2)) * valid_depth_mask
        diff_depth_l1 = torch.abs((rastered_depth - gt_depth) * presence_sil_mask) * valid_depth_mask
    else:
        diff_depth_rmse = torch.sqrt(((rastered_depth - gt_depth)) ** 2) * valid_depth_mask
        diff_depth_l1 = torch.abs((rastered_depth - gt_depth)) * valid_depth_mask
    rmse = diff_depth_rmse.sum() / valid_depth_mask.sum()
    depth_l1 = diff_depth_l1.sum() / valid_depth_mask.sum()
    return np.array([psnr.item(), depth_l1.item(), rmse.item()], dtype=np.float64)


def main():
    g = np.random.default_rng(21)
    out = {}
    for name, (H, W, use_sil, exact_channel) in {"sil_64x80": (64, 80, True, None), "nosil_37x53": (37, 53, False, None),
                                                  "exact_g_48x64": (48, 64, False, 1)}.items():
        gt_im = g.random((3, H, W)).astype(np.float32)
        im = np.clip(gt_im + g.normal(0, 0.05, gt_im.shape), 0, 1).astype(np.float32)
        if exact_channel is not None:
            im[exact_channel] = gt_im[exact_channel]        # mse 0 in that channel: PSNR +inf
        gt_depth = (g.random((1, H, W)) * 5 + 0.5).astype(np.float32)
        gt_depth[g.random((1, H, W)) < 0.15] = 0.0          # invalid gt depth
        depth = (gt_depth + g.normal(0, 0.1, gt_depth.shape)).astype(np.float32)
        opac = g.random((1, H, W)).astype(np.float32)
        sil_thres = 0.5
        t = [torch.tensor(a) for a in (im, gt_im, depth, gt_depth, opac)]
        res = reference_terms(*t, sil_thres, use_sil)
        for k, v in (("im", im), ("gt_im", gt_im), ("depth", depth), ("gt_depth", gt_depth), ("final_opacity", opac)):
            out[name + "/" + k] = v
        out[name + "/sil_thres"] = np.float32(sil_thres)
        out[name + "/use_sil"] = np.int32(use_sil)
        out[name + "/expect"] = res
    os.makedirs(os.path.join(HERE, "eval"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "eval", "psnr_depth.npz"), **out)


if __name__ == "__main__":
    main()
