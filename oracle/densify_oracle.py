"""CPU restatement (numpy) of the numeric part of the reference's silhouette densification — TEST INFRASTRUCTURE ONLY.

Only tests/ may import this file; the product path (hier-slam_amd/csrc/hsr_densify.hip behind include/hsr_densify.h) never does.
PARITY UNPINNED by reference outputs: add_new_gaussians_semantic and get_pointcloud allocate on 'cuda' (scripts/hierslam.py:153,
:165, :1286) and scripts/hierslam.py cannot be imported here (cv2, wandb, ...); pinned by tests/test_densify.py against the same
lines written with torch CPU ops (torch.median, boolean-mask indexing, torch.inverse).

Follows scripts/hierslam.py:1271-1278 (non-presence mask), :1289-1290 (valid depth), :144-194 (get_pointcloud, "projective"
mean_sq_dist), :1157 (log_scales)."""
import numpy as np


def non_presence_points(silhouette, render_depth, gt_depth, color, intrinsics, c2w, sil_thres, depth_factor=50.0, dtype=np.float32):
    f = lambda a: np.asarray(a, dtype=dtype)
    sil, rd, gt, col = f(silhouette), f(render_depth), f(gt_depth), f(color)
    H, W = gt.shape
    with np.errstate(invalid="ignore"):                              # inf * 0 is the NaN the reference gets too
        derr = np.abs(gt - rd) * (gt > 0)
    # torch.median: NaN if any error is NaN, otherwise the lower median (rank (n - 1) // 2)
    med = dtype(np.nan) if np.isnan(derr).any() else np.sort(derr.reshape(-1))[(derr.size - 1) // 2]
    mask = (sil < dtype(sil_thres)) | ((rd > gt) & (derr > dtype(depth_factor) * med))
    mask = (mask & (gt > 0)).reshape(-1)
    K = f(intrinsics)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    xg, yg = np.meshgrid(np.arange(W, dtype=dtype), np.arange(H, dtype=dtype), indexing="xy")
    xx, yy = ((xg - cx) / fx).reshape(-1), ((yg - cy) / fy).reshape(-1)
    z = gt.reshape(-1)
    pc = np.stack([xx * z, yy * z, z], axis=1)
    M = f(c2w)
    pts = ((pc[:, 0:1] * M[None, :3, 0] + pc[:, 1:2] * M[None, :3, 1]) + pc[:, 2:3] * M[None, :3, 2]) + M[None, :3, 3]
    sg = z / ((fx + fy) / dtype(2))
    msd = sg * sg
    cols = col.reshape(3, -1).T
    return {"mask": mask, "median": med, "means3D": pts[mask], "rgb": cols[mask], "mean3_sq_dist": msd[mask],
            "log_scales": np.log(np.sqrt(msd[mask]))}
