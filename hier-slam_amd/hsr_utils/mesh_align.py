"""A run's mesh registered to the ground truth before it is scored, on the device (include/align/hsr_mesh_align.h):
rigid point-to-point ICP with a correspondence distance and an identity start, which is what the evaluation behind this family's
published tables does through Open3D (registration_icp with TransformationEstimationPointToPoint).  Open3D is not a dependency and
the reference has no mesh evaluation, so the loop is restated here and not pinned by Open3D's outputs.

    rigid_from_sums(sums)                                       host float64: Horn's closed form (evaluate._align) from the 17 sums
    icp_step(grid, source, transform, max_dist, correspondences=False)      ONE hsr_icp_step; nothing is read back
    icp(source, target, max_dist=0.1, init=None, max_iterations=30, ...)    the loop: one step and ONE host read of 136 bytes a pass
    trajectory_alignment(gt_w2cs, est_w2cs)                     host float64 [4,4]: the estimate's world -> the ground truth's, from camera centres
    transform_points(points, T)                                 the kernel's float32 chain in plain torch
    align_mesh(rec, gt, n_samples=200000, seed=0, **icp_kw)     surface samples of both, icp, the aligned vertices

There is no CPU path for anything that launches; rigid_from_sums and trajectory_alignment are host numpy and run anywhere.
"""
import numpy as np
import torch

from diff_gaussian_rasterization import _abi

from .mesh_eval import NearestGrid, _device_tensor, _host, _mesh, sample_mesh

_lib = _abi.lib

SUMS = 17      # HSR_ICP_SUMS


def _matrix(T, what="transform"):
    """T as a float64 [4,4]; a [3,4] gets the row 0 0 0 1"""
    m = np.asarray(_host(T), dtype=np.float64)
    if m.shape == (3, 4):
        m = np.concatenate([m, [[0.0, 0.0, 0.0, 1.0]]])
    if m.shape != (4, 4):
        raise RuntimeError("hsr_utils.mesh_align: %s must be [4,4] or [3,4] (got %s)" % (what, m.shape))
    if not np.isfinite(m).all():
        raise ValueError("hsr_utils.mesh_align: %s holds an entry that is not finite" % what)
    return m


def rigid_from_sums(sums):
    """(R float64 [3,3], t float64 [3]) with R p' + t ~ q in the least-squares sense, from the 17 sums of hsr_icp_step: n = s[0],
    mp = s[1:4] / n, mq = s[4:7] / n, W = s[7:16] as [3,3] - n mp mq^T, the SVD of W^T with the determinant's sign on the last singular
    direction (evaluate._align, the closed form trajectory_ate uses), t = mq - R mp.  ValueError below three correspondences."""
    s = np.asarray(_host(sums), dtype=np.float64).reshape(-1)
    if s.shape[0] != SUMS:
        raise RuntimeError("hsr_utils.mesh_align: sums must hold %d numbers (got %d)" % (SUMS, s.shape[0]))
    n = s[0]
    if not n >= 3:
        raise ValueError("hsr_utils.mesh_align: %d correspondences; a rigid motion needs three" % (0 if not n > 0 else int(n)))
    mp, mq = s[1:4] / n, s[4:7] / n
    W = s[7:16].reshape(3, 3) - n * np.outer(mp, mq)
    U, _d, Vh = np.linalg.svd(W.T)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vh) < 0:
        S[2, 2] = -1
    R = U @ S @ Vh
    return R, mq - R @ mp


def icp_step(grid, source, transform, max_dist, correspondences=False):
    """ONE hsr_icp_step of `source` (float32 [N,3] on grid.device) under `transform` ([4,4] or [3,4], rounded to float32) against the
    points of `grid` (a NearestGrid): the device tensor float64 [17] of the header's sums, and with correspondences=True also
    (d2 float32 [N], index int32 [N]) — (+inf, -1) where the nearest target is farther than max_dist.  Nothing is read back."""
    if not isinstance(grid, NearestGrid):
        raise RuntimeError("hsr_utils.mesh_align: grid must be a NearestGrid")
    src = _device_tensor(source, "source", torch.float32, 3, grid.device)
    m = np.ascontiguousarray(_matrix(transform)[:3].astype(np.float32)).reshape(12)
    max_dist = float(max_dist)
    if not (np.isfinite(max_dist) and max_dist > 0):
        raise ValueError("hsr_utils.mesh_align: max_dist must be finite and positive (got %r)" % max_dist)
    N, dev = src.shape[0], grid.device
    sums = torch.empty(SUMS, dtype=torch.float64, device=dev)
    scratch_bytes = _lib.hsr_icp_scratch_bytes(N)
    scratch = torch.empty(max(1, scratch_bytes // 8), dtype=torch.float64, device=dev)
    d2 = torch.empty(N, dtype=torch.float32, device=dev) if correspondences else None
    index = torch.empty(N, dtype=torch.int32, device=dev) if correspondences else None
    _abi.call(_lib.hsr_icp_step, "hsr_icp_step", dev, *grid.dims, *grid.origin, grid.cell, grid.M, grid.cell_start.data_ptr(),
              grid.packed.data_ptr(), N, src.data_ptr(), m.ctypes.data_as(_abi.fp), max_dist,
              None if index is None else index.data_ptr(), None if d2 is None else d2.data_ptr(), sums.data_ptr(), scratch.data_ptr(),
              scratch_bytes)
    return (sums, d2, index) if correspondences else sums


def transform_points(points, T):
    """float32 device points [N,3] through T ([4,4] or [3,4], rounded to float32) by the kernel's own chain,
    x' = ((m00 * x + m01 * y) + m02 * z) + m03 and likewise y' and z', every operation rounded once: separate multiplies and adds in
    plain torch, nothing fused."""
    p = _device_tensor(points, "points", torch.float32, 3)
    m = _matrix(T)[:3].astype(np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    rows = []
    for r in range(3):
        a, b, c = x * float(m[r, 0]), y * float(m[r, 1]), z * float(m[r, 2])
        rows.append(((a + b) + c) + float(m[r, 3]))
    return torch.stack(rows, dim=1)


def icp(source, target, max_dist=0.1, init=None, max_iterations=30, relative_fitness=1e-6, relative_rmse=1e-6, cell=None):
    """Rigid point-to-point ICP of `source` (float32 [N,3]) onto `target` (a NearestGrid, or points float32 [M,3] that are put into one
    with cells of `cell`, default max_dist), the loop of Open3D's registration_icp with TransformationEstimationPointToPoint restated:
    T = init (float64 [4,4], default the identity); every pass makes ONE icp_step of the ORIGINAL points under T rounded to float32 and
    ONE host read of the 17 sums; fitness = count / N, inlier_rmse = sqrt(sum d2 / count); it stops as converged when both changed by
    less than relative_fitness and relative_rmse since the previous pass, and after max_iterations updates; otherwise
    T = [R t; 0 1] @ T with rigid_from_sums' R and t.  T is composed in float64 on the host and the points are never transformed
    cumulatively.  The source is sorted once, by its cells under init.  Returns dict(transform float64 [4,4], fitness, inlier_rmse,
    iterations, converged); the numbers are the last pass's and so belong to `transform`.  ValueError when a pass has fewer than three
    correspondences."""
    max_dist = float(max_dist)
    if not (np.isfinite(max_dist) and max_dist > 0):
        raise ValueError("hsr_utils.mesh_align: max_dist must be finite and positive (got %r)" % max_dist)
    max_iterations = int(max_iterations)
    if max_iterations < 0:
        raise ValueError("hsr_utils.mesh_align: max_iterations must be >= 0 (got %d)" % max_iterations)
    T = np.eye(4) if init is None else _matrix(init, "init").copy()
    if isinstance(target, NearestGrid):
        grid = target
    else:
        grid = NearestGrid(_device_tensor(target, "target", torch.float32, 3), max_dist if cell is None else cell)
    src = _device_tensor(source, "source", torch.float32, 3, grid.device)
    N = src.shape[0]
    if N < 3:
        raise ValueError("hsr_utils.mesh_align: %d source points; a rigid motion needs three" % N)
    src = src[torch.sort(grid._cells(transform_points(src, T)), stable=True).indices].contiguous()      # once: a pass moves a point by a fraction of a cell
    previous, iterations, converged = None, 0, False
    while True:
        s = icp_step(grid, src, T, max_dist).cpu().numpy()      # the one host read of the pass: 136 bytes
        if s[0] < 3:
            raise ValueError("hsr_utils.mesh_align: %d correspondences within %g of the target at pass %d; a rigid motion needs three"
                             % (int(s[0]), max_dist, iterations))
        fitness, rmse = float(s[0]) / N, float(np.sqrt(s[16] / s[0]))
        if previous is not None and abs(previous[0] - fitness) < relative_fitness and abs(previous[1] - rmse) < relative_rmse:
            converged = True
            break
        if iterations >= max_iterations:
            break
        R, t = rigid_from_sums(s)
        update = np.eye(4)
        update[:3, :3], update[:3, 3] = R, t
        T = update @ T
        previous, iterations = (fitness, rmse), iterations + 1
    return dict(transform=T, fitness=fitness, inlier_rmse=rmse, iterations=iterations, converged=converged)


def trajectory_alignment(gt_w2cs, est_w2cs):
    """float64 [4,4]: the rigid map from the estimate's world to the ground truth's, Horn's closed form (evaluate._align) on the CAMERA
    CENTRES, -R^T t of each world-to-camera matrix — not on the [:3,3] columns that evaluate.trajectory_ate aligns: that alignment lives
    in camera space and cannot be applied to a mesh.  Frames whose ground-truth pose holds a NaN are skipped; the ground truth may be
    longer than the estimate.  ValueError below three usable frames.  Host numpy."""
    from .evaluate import _align
    gts = [np.asarray(_host(m), dtype=np.float64) for m in gt_w2cs]
    ests = [np.asarray(_host(m), dtype=np.float64) for m in est_w2cs]
    if len(ests) < 1 or len(gts) < len(ests):
        raise RuntimeError("hsr_utils.mesh_align: %d estimated poses for %d gt poses" % (len(ests), len(gts)))
    centre = lambda m: -m[:3, :3].T @ m[:3, 3]
    pairs = [(centre(g), centre(e)) for g, e in zip(gts, ests) if not np.isnan(g).any()]
    if len(pairs) < 3:
        raise ValueError("hsr_utils.mesh_align: %d frames with a ground-truth pose; a rigid motion needs three" % len(pairs))
    gt_c, est_c = np.stack([p[0] for p in pairs]).T, np.stack([p[1] for p in pairs]).T
    rot, trans, _err = _align(est_c, gt_c)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot, trans.reshape(3)
    return T


def align_mesh(rec, gt, n_samples=200000, seed=0, **icp_kw):
    """(the vertices of `rec` registered to `gt`, icp's dictionary): rec and gt are (vertices, faces[, ...]); n_samples points are drawn
    on each surface — sample_mesh with seed + 2 and seed + 3, so that they are not the samples mesh_metrics scores with — and
    icp(rec samples -> gt samples, **icp_kw) gives the transform the vertices go through (transform_points).  Surface samples, not
    vertices: they do not depend on the tessellation; a caller who wants vertices calls icp."""
    dev = rec[0].device if isinstance(rec[0], torch.Tensor) and rec[0].is_cuda else torch.device("cuda", torch.cuda.current_device())
    rv, rf, _ = _mesh(rec[0], rec[1], device=dev)
    gv, gf, _ = _mesh(gt[0], gt[1], device=dev)
    n = int(n_samples)
    if n < 3:
        raise ValueError("hsr_utils.mesh_align: n_samples must be >= 3")
    ps = sample_mesh(rv, rf, n, int(seed) + 2)[0]
    pt = sample_mesh(gv, gf, n, int(seed) + 3)[0]
    result = icp(ps, pt, **icp_kw)
    return transform_points(rv, result["transform"]), result


__all__ = ["rigid_from_sums", "icp_step", "icp", "trajectory_alignment", "transform_points", "align_mesh"]
