"""A run's mesh scored against a ground-truth mesh, on the device (include/eval/hsr_mesh_eval.h): what the reference
family reports with Open3D, trimesh or a KD-tree after a run — accuracy, completion, completion ratio and, for a semantic system, the 3D
mIoU of labels transferred by nearest neighbour — after culling the ground truth to what the cameras saw.  The reference itself has no
mesh evaluation, so the rules are this project's own and the header states each of them.

    sample_mesh(vertices, faces, n, seed=0, labels=None)      hsr_mesh_areas, torch.cumsum, ONE host read (the total area), hsr_mesh_sample
    NearestGrid(points, cell)                                  hsr_nn_cells, torch.sort, torch.searchsorted, hsr_nn_pack; ONE host read (the box)
        .query(q)                                              hsr_nn_cells, torch.sort, ONE hsr_nn_query: exact (d2, index), no host read
    seen_vertices(vertices, w2cs, intrinsics, H, W, depths=None, eps=0.0)      ONE hsr_mesh_seen per view
    cull_mesh(vertices, faces, seen, *per_vertex)              plain torch
    mesh_metrics(rec, gt, n_samples=200000, threshold=0.05, seed=0, num_classes=None)
    evaluate_mesh_run(params, gt_ply, voxel_size=, every=5, ...)    mesh_run's mesh, the culled ground truth, mesh_metrics; with
                                                               depth_views=N also mesh_depth.mesh_depth_l1 from N virtual views, and with
                                                               align="icp" | "trajectory" the run's mesh registered first (mesh_align)

There is no CPU path for anything that launches; cull_mesh is plain torch and runs anywhere.
"""
import os
import tempfile

import numpy as np
import torch

from diff_gaussian_rasterization import _abi

_lib = _abi.lib

MAX_IMAGE_SIDE = 16384      # HSR_MESH_MAX_IMAGE_SIDE
MAX_SIDE = 1024             # HSR_NN_MAX_SIDE
MAX_CELLS = 2 ** 24         # HSR_NN_MAX_CELLS
MAX_ITEMS = 2 ** 31 - 1


def _host(m):
    return m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)


def _device_tensor(t, what, dtype, cols=None, device=None):
    """t as a contiguous device tensor of `dtype`, [n] or [n, cols]; arrays are copied to `device`"""
    if not isinstance(t, torch.Tensor):
        if device is None:
            raise RuntimeError("hsr_utils.mesh_eval: %s must be a tensor on a HIP device; there is no CPU path" % what)
        t = torch.as_tensor(np.ascontiguousarray(_host(t)), device=device)
    if not t.is_cuda:
        if device is None:
            raise RuntimeError("hsr_utils.mesh_eval: %s must be a tensor on a HIP device; there is no CPU path" % what)
        t = t.to(device)
    if device is not None and t.device != device:
        raise RuntimeError("hsr_utils.mesh_eval: %s is on %s, not on %s" % (what, t.device, device))
    want = (t.dim() == 1) if cols is None else (t.dim() == 2 and t.shape[1] == cols)
    if not want or t.shape[0] > MAX_ITEMS:
        raise RuntimeError("hsr_utils.mesh_eval: %s must be %s (got %s)" % (what, "[n]" if cols is None else "[n,%d]" % cols, tuple(t.shape)))
    return t.detach().to(dtype).contiguous()


def _mesh(vertices, faces, labels=None, device=None):
    v = _device_tensor(vertices, "vertices", torch.float32, 3, device)
    f = _device_tensor(faces, "faces", torch.int32, 3, v.device)
    lab = None if labels is None else _device_tensor(labels, "labels", torch.int32, None, v.device)
    if lab is not None and lab.shape[0] != v.shape[0]:
        raise RuntimeError("hsr_utils.mesh_eval: labels must be [V] = [%d] (got %s)" % (v.shape[0], tuple(lab.shape)))
    return v, f, lab


# ---- areas and samples --------------------------------------------------------------------------------------------------------------------
def face_areas(vertices, faces):
    """float32 [F]: the area of every face; 0 for a face with an index outside the vertices or an area that is not finite"""
    v, f, _ = _mesh(vertices, faces)
    if v.shape[0] == 0:
        return torch.zeros(f.shape[0], dtype=torch.float32, device=v.device)
    area = torch.empty(f.shape[0], dtype=torch.float32, device=v.device)
    _abi.call(_lib.hsr_mesh_areas, "hsr_mesh_areas", v.device, v.shape[0], f.shape[0], v.data_ptr(), f.data_ptr(), area.data_ptr())
    return area


def _sample(v, f, lab, n, seed):
    """(points, face, labels | None, total area as a float): the one host read is the total"""
    n = int(n)
    if n < 0 or n > MAX_ITEMS:
        raise ValueError("hsr_utils.mesh_eval: the number of samples must be 0..2^31-1 (got %d)" % n)
    if f.shape[0] == 0 or v.shape[0] == 0:
        raise ValueError("hsr_utils.mesh_eval: the mesh has no faces")
    cum = torch.cumsum(face_areas(v, f).double(), 0)
    total = float(cum[-1])      # the one host read
    if not (total > 0 and np.isfinite(total)):
        raise ValueError("hsr_utils.mesh_eval: the mesh has a total area of %g; nothing to sample" % total)
    dev = v.device
    points = torch.empty((n, 3), dtype=torch.float32, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    out_label = None if lab is None else torch.empty(n, dtype=torch.int32, device=dev)
    _abi.call(_lib.hsr_mesh_sample, "hsr_mesh_sample", dev, v.shape[0], f.shape[0], n, int(seed) % 2 ** 64, v.data_ptr(), f.data_ptr(),
              cum.data_ptr(), None if lab is None else lab.data_ptr(), points.data_ptr(), face.data_ptr(),
              None if out_label is None else out_label.data_ptr())
    return points, face, out_label, total


def sample_mesh(vertices, faces, n, seed=0, labels=None):
    """n points on the surface, the faces drawn in proportion to their areas from a counter-based generator: (points float32 [n,3],
    face int32 [n], labels int32 [n] | None), on the device, the same for the same seed.  labels int32 [V]: a sample takes the label
    of its nearest corner in barycentric terms.  ValueError on a mesh without faces or without area.  One host read (the total area)."""
    if len(faces) == 0 or len(vertices) == 0:
        raise ValueError("hsr_utils.mesh_eval: the mesh has no faces")
    v, f, lab = _mesh(vertices, faces, labels)
    return _sample(v, f, lab, n, seed)[:3]


# ---- nearest neighbours -------------------------------------------------------------------------------------------------------------------
class NearestGrid:
    """The points float32 [M,3] in a uniform grid of cells of size `cell` over the box of the finite points, packed cell by cell:
    .query(q) is then the EXACT nearest neighbour of every query among ALL the points (the header defines it by brute force), found by
    walking the rings of cells around the query.  .origin, .cell, .dims = (X, Y, Z) are the grid; the cell is grown in steps of 2 %
    until every side is <= 1024 and X * Y * Z <= 2^24.  ValueError when no point is finite.  One host read (the box)."""

    def __init__(self, points, cell):
        c = float(cell)
        if not (np.isfinite(c) and c > 0):
            raise ValueError("hsr_utils.mesh_eval: cell must be finite and positive (got %r)" % (cell,))
        pts = points if isinstance(points, torch.Tensor) else torch.as_tensor(np.asarray(points))
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise RuntimeError("hsr_utils.mesh_eval: points must be [n,3] (got %s)" % (tuple(pts.shape),))
        pts = pts.detach().to(torch.float32)
        M = pts.shape[0]
        finite = torch.isfinite(pts).all(dim=1, keepdim=True) if M else None
        box = None
        if M:      # wherever the points are: the refusal below needs no device
            inf = torch.full_like(pts, float("inf"))
            box = torch.stack([torch.where(finite, pts, inf).min(dim=0).values, torch.where(finite, pts, -inf).max(dim=0).values])
            box = box.cpu().numpy().astype(np.float64)      # the one host read
        if box is None or not np.isfinite(box).all():
            raise ValueError("hsr_utils.mesh_eval: no finite point to search among")
        pts = _device_tensor(pts, "points", torch.float32, 3)
        dev = pts.device
        extent = box[1] - box[0]

        def sides(step):
            step = float(np.float32(step))      # what the kernels divide by
            return [int(np.floor(e / step)) + 1 for e in extent]

        while max(sides(c)) > MAX_SIDE or float(np.prod([float(s) for s in sides(c)])) > MAX_CELLS:
            c *= 1.02
        self.cell = float(np.float32(c))
        self.dims = tuple(sides(c))
        self.origin = tuple(float(np.float32(o)) for o in box[0])
        self.device, self.M = dev, M
        cells = self._cells(pts)
        sorted_cells, order = torch.sort(cells, stable=True)
        X, Y, Z = self.dims
        self.cell_start = torch.searchsorted(sorted_cells, torch.arange(X * Y * Z + 1, dtype=torch.int32, device=dev)).to(torch.int32)
        self.packed = torch.empty((M, 4), dtype=torch.float32, device=dev)
        _abi.call(_lib.hsr_nn_pack, "hsr_nn_pack", dev, M, pts.data_ptr(), order.data_ptr(), self.packed.data_ptr())

    def _cells(self, pts):
        cells = torch.empty(pts.shape[0], dtype=torch.int32, device=self.device)
        _abi.call(_lib.hsr_nn_cells, "hsr_nn_cells", self.device, *self.dims, *self.origin, self.cell, pts.shape[0], pts.data_ptr(), cells.data_ptr())
        return cells

    def query(self, q):
        """(d2 float32 [N], index int32 [N]): the least squared distance from every query to the points and the smallest index that
        reaches it; (+inf, -1) for a query with a NaN or when nothing is at a finite distance.  The queries go to the kernel in the
        order of their own cells, so that a wave's lanes walk the same cells, and the answers are scattered back.  No host read."""
        q = _device_tensor(q, "queries", torch.float32, 3, self.device)
        N = q.shape[0]
        d2 = torch.empty(N, dtype=torch.float32, device=self.device)
        index = torch.empty(N, dtype=torch.int32, device=self.device)
        if N == 0:
            return d2, index
        order = torch.sort(self._cells(q), stable=True).indices
        qs = q[order].contiguous()
        d2s, indexs = torch.empty_like(d2), torch.empty_like(index)
        _abi.call(_lib.hsr_nn_query, "hsr_nn_query", self.device, *self.dims, *self.origin, self.cell, self.M, self.cell_start.data_ptr(),
                  self.packed.data_ptr(), N, qs.data_ptr(), d2s.data_ptr(), indexs.data_ptr())
        d2[order] = d2s
        index[order] = indexs
        return d2, index


# ---- what the cameras saw -----------------------------------------------------------------------------------------------------------------
def seen_vertices(vertices, w2cs, intrinsics, H, W, depths=None, eps=0.0):
    """bool [V] on the device: the vertices that at least one view saw.  w2cs [T,4,4] world-to-camera matrices (host or device: one
    copy), intrinsics [3,3], the image H x W; a vertex is seen by a view when it lies in front of the camera and projects into the
    image and, with depths (T planes float32 [H,W] or [1,H,W] on the device, z along the camera's axis), its pixel's depth d is
    positive and finite and the vertex is no deeper than d + eps.  One launch per view, nothing read back."""
    H, W = int(H), int(W)
    if not (1 <= H <= MAX_IMAGE_SIDE and 1 <= W <= MAX_IMAGE_SIDE):
        raise ValueError("hsr_utils.mesh_eval: the image is %d x %d; sides are 1..%d" % (W, H, MAX_IMAGE_SIDE))
    eps = float(eps)
    if not (np.isfinite(eps) and eps >= 0):
        raise ValueError("hsr_utils.mesh_eval: eps must be finite and not negative (got %r)" % eps)
    v = _device_tensor(vertices, "vertices", torch.float32, 3)
    views = np.ascontiguousarray(_host(w2cs), dtype=np.float32)
    k = _host(intrinsics)
    if views.ndim != 3 or views.shape[1:] != (4, 4) or k.ndim != 2 or k.shape[0] < 3 or k.shape[1] < 3:
        raise RuntimeError("hsr_utils.mesh_eval: w2cs must be [T,4,4] and intrinsics [3,3] (got %s and %s)" % (views.shape, k.shape))
    if depths is not None and len(depths) != len(views):
        raise RuntimeError("hsr_utils.mesh_eval: %d depth planes for %d views" % (len(depths), len(views)))
    seen = torch.zeros(v.shape[0], dtype=torch.uint8, device=v.device)
    for t, m in enumerate(views):
        depth = None
        if depths is not None:
            depth = depths[t]
            if not isinstance(depth, torch.Tensor) or depth.device != v.device or depth.dtype != torch.float32 or depth.numel() != H * W \
                    or tuple(depth.shape[-2:]) != (H, W):
                raise RuntimeError("hsr_utils.mesh_eval: depth %d must be a float32 tensor [%d,%d] on %s" % (t, H, W, v.device))
            depth = depth.detach().contiguous()
        _abi.call(_lib.hsr_mesh_seen, "hsr_mesh_seen", v.device, v.shape[0], v.data_ptr(), H, W, float(k[0][0]), float(k[1][1]), float(k[0][2]),
                  float(k[1][2]), m.ctypes.data_as(_abi.fp), None if depth is None else depth.data_ptr(), eps, seen.data_ptr())
    return seen.bool()


def cull_mesh(vertices, faces, seen, *per_vertex):
    """(vertices, faces, *per_vertex) without what was not seen: a face stays when all three of its vertices were seen, the seen
    vertices stay, and the faces are re-indexed.  Plain torch, on whatever device the tensors are; None among per_vertex stays None."""
    seen = seen.bool()
    faces = faces.long()
    kept = faces[seen[faces].all(dim=1)] if faces.shape[0] else faces
    new_index = torch.cumsum(seen.to(torch.int64), 0) - 1
    out_faces = new_index[kept].to(torch.int32)
    return (vertices[seen], out_faces) + tuple(None if p is None else p[seen] for p in per_vertex)


# ---- the numbers --------------------------------------------------------------------------------------------------------------------------
def distance_metrics(d2_rec, d2_gt, threshold):
    """the six distance numbers of mesh_metrics from the squared distances rec -> gt and gt -> rec: float64 0-dim tensors"""
    da, dc = torch.sqrt(d2_rec.double()), torch.sqrt(d2_gt.double())
    accuracy, completion = da.mean(), dc.mean()
    ra, rc = (da <= threshold).double().mean(), (dc <= threshold).double().mean()
    f = torch.where(ra + rc > 0, 2 * ra * rc / torch.clamp_min(ra + rc, 1e-300), torch.zeros_like(ra))
    return dict(accuracy=accuracy, completion=completion, accuracy_ratio=ra, completion_ratio=rc, f_score=f, chamfer=0.5 * (accuracy + completion))


def label_metrics(gt_labels, rec_labels, nearest, num_classes):
    """confusion int64 [C,C] (gt label x label of the nearest rec sample), label_accuracy and miou (over the classes with G + P > 0)
    from the labels of the gt samples, of the rec samples and the index of each gt sample's nearest rec sample.  A negative label, a
    label >= C and a gt sample without a neighbour are ignored."""
    C = int(num_classes)
    has = nearest >= 0
    pred = torch.where(has, rec_labels[nearest.clamp_min(0).long()], torch.full_like(gt_labels, -1)).long()
    g = gt_labels.long()
    ok = (g >= 0) & (g < C) & (pred >= 0) & (pred < C)
    confusion = torch.bincount(torch.where(ok, g * C + pred, torch.full_like(g, C * C)), minlength=C * C + 1)[:C * C].reshape(C, C)
    inter = confusion.diagonal().double()
    G, P = confusion.sum(dim=1).double(), confusion.sum(dim=0).double()
    union = G + P - inter
    present = (G + P) > 0
    iou = torch.where(present, inter / torch.clamp_min(union, 1.0), torch.zeros_like(inter))
    return dict(confusion=confusion, label_accuracy=inter.sum() / torch.clamp_min(confusion.sum().double(), 1.0),
                miou=iou.sum() / torch.clamp_min(present.double().sum(), 1.0))


def mesh_metrics(rec, gt, n_samples=200000, threshold=0.05, seed=0, num_classes=None):
    """A reconstructed mesh against a ground-truth one, both (vertices, faces[, labels]) in one world frame, in metres.  n_samples
    points are drawn on each (sample_mesh with seed and seed + 1) and each side's nearest neighbour on the other is found exactly
    (NearestGrid, its cell twice the samples' mean spacing sqrt(area / n)).  Returns float64 0-dim device tensors, each from
    sqrt(d2.double()):
        accuracy      mean distance rec -> gt            accuracy_ratio     share of rec samples within threshold
        completion    mean distance gt -> rec            completion_ratio   share of gt samples within threshold
        f_score       harmonic mean of the two ratios (0 when both are 0)   chamfer   mean of accuracy and completion
    and, with labels (int [V], negative: ignored) on both sides, confusion int64 [C,C] (gt label x label of the nearest rec sample),
    label_accuracy and miou over the classes with G + P > 0; C = num_classes, or 1 + the largest label (one more host read).
    threshold = 0.05 and n_samples = 200000 are the family's conventions.  Host reads: each side's total area and each grid's box."""
    n = int(n_samples)
    if n < 1:
        raise ValueError("hsr_utils.mesh_eval: n_samples must be >= 1")
    threshold = float(threshold)
    dev = rec[0].device if isinstance(rec[0], torch.Tensor) and rec[0].is_cuda else torch.device("cuda", torch.cuda.current_device())
    rv, rf, rl = _mesh(*rec, device=dev)
    gv, gf, gl = _mesh(*gt, device=dev)
    pr, _fr, lr, area_r = _sample(rv, rf, rl, n, seed)
    pg, _fg, lg, area_g = _sample(gv, gf, gl, n, int(seed) + 1)
    d2_rec, _ = NearestGrid(pg, 2.0 * np.sqrt(area_g / n)).query(pr)
    d2_gt, nearest = NearestGrid(pr, 2.0 * np.sqrt(area_r / n)).query(pg)
    out = distance_metrics(d2_rec, d2_gt, threshold)
    if lr is not None and lg is not None:
        if num_classes is None:
            num_classes = int(torch.maximum(rl.max(), gl.max())) + 1      # one more host read
        out.update(label_metrics(lg, lr, nearest, max(1, int(num_classes))))
    return out


# ---- a run --------------------------------------------------------------------------------------------------------------------------------
def evaluate_mesh_run(params, gt_ply, *, voxel_size, every=5, threshold=0.05, n_samples=200000, seed=0, semantic=False, num_classes=None,
                      sil_thres=0.5, cull=True, keep_mesh=None, intrinsics=None, width=None, height=None, num_frames=None, cam=None,
                      first_frame_w2c=None, near=0.01, far=100, depth_views=0, depth_seed=0, depth_size=None, align=None, align_max_dist=0.1,
                      align_iterations=30, gt_w2cs=None, **mesh_kw):
    """The mesh of a finished run scored against the ground-truth mesh of its scene.  mesh.mesh_run(params, voxel_size=, every=,
    semantic=, ...) makes the run's mesh (kept at keep_mesh when that is a path); gt_ply is read with mesh.load_mesh_ply; with cull=True
    the ground truth is culled to the vertices seen from every `every`-th estimated pose — in the image, and no deeper than the map's
    rendered depth there plus eps = threshold, where the rendered opacity exceeds sil_thres — and mesh_metrics(rec, gt, n_samples,
    threshold, seed, num_classes) scores the two; labels count with semantic=True when the ground truth carries them.  params,
    intrinsics, width, height, num_frames, cam, first_frame_w2c, near and far are mesh_run's, as is every other keyword (label_mode,
    depth_max, bounds, ...).  Returns mesh_metrics' dictionary plus the integers rec_vertices, rec_faces, gt_vertices, gt_faces,
    gt_vertices_seen and gt_faces_kept.  With depth_views = N > 0 the (culled) ground truth and the run's mesh are also rendered to depth
    from N views the sensor never took — mesh_depth.virtual_views(the poses that were meshed, the culled ground truth's vertices, N,
    depth_seed) — at depth_size = (H, W), or the run's own size, with the intrinsics scaled per axis, and mesh_depth.mesh_depth_l1 adds
    depth_l1, depth_l1_covered, depth_gt_cover, depth_rec_cover (floats) and depth_views; with the default 0 no key is added.
    align registers the run's mesh to the ground truth (mesh_align; include/align/hsr_mesh_align.h)
    AFTER the cull (which keeps using the estimated poses) and BEFORE mesh_metrics and Depth L1, which then see the aligned vertices:
    "icp" is mesh_align.align_mesh(the run's mesh, the culled ground truth, n_samples, seed, max_dist=align_max_dist,
    max_iterations=align_iterations) and "trajectory" applies mesh_align.trajectory_alignment(gt_w2cs, the run's poses), which needs
    gt_w2cs [T,4,4] world-to-camera; either adds align, align_transform (a nested list, estimate's world -> ground truth's) and, for
    "icp" only, align_fitness, align_rmse and align_iterations.  With the default None nothing is called and no key is added."""
    if align not in (None, "icp", "trajectory"):
        raise ValueError("hsr_utils.mesh_eval: align must be None, \"icp\" or \"trajectory\" (got %r)" % (align,))
    if align == "trajectory" and gt_w2cs is None:
        raise ValueError("hsr_utils.mesh_eval: align=\"trajectory\" needs gt_w2cs, the ground-truth world-to-camera matrices")
    from . import mesh, slam
    from .camera import setup_camera
    from .replay import run_w2cs
    dev = params['means3D'].device
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "run.ply") if keep_mesh is None else keep_mesh
        mesh.mesh_run(params, path, voxel_size=voxel_size, every=every, semantic=semantic, sil_thres=sil_thres, intrinsics=intrinsics, width=width,
                      height=height, num_frames=num_frames, cam=cam, first_frame_w2c=first_frame_w2c, near=near, far=far, **mesh_kw)
        rec_v, rec_f, _rgb, rec_l = mesh.load_mesh_ply(path)
    gt_v, gt_f, _rgb, gt_l = mesh.load_mesh_ply(gt_ply)
    if len(rec_f) == 0 or len(gt_f) == 0:
        raise ValueError("hsr_utils.mesh_eval: %s has no faces" % ("the run's mesh" if len(rec_f) == 0 else gt_ply))
    use_labels = bool(semantic) and rec_l is not None and gt_l is not None
    gv, gf, gl = _mesh(gt_v, gt_f, gt_l if use_labels else None, device=dev)
    counts = dict(rec_vertices=len(rec_v), rec_faces=len(rec_f), gt_vertices=len(gt_v), gt_faces=len(gt_f), gt_vertices_seen=len(gt_v),
                  gt_faces_kept=len(gt_f))
    depth_views = int(depth_views)
    if depth_views < 0:
        raise ValueError("hsr_utils.mesh_eval: depth_views must be >= 0 (got %d)" % depth_views)
    if cull or depth_views or align == "trajectory":
        # the views of mesh_run: the same camera, the same poses, the same silhouette
        k = np.asarray(_host(params['intrinsics'] if intrinsics is None else intrinsics), dtype=np.float32)[:3, :3]
        w = int(_host(params['org_width'])) if width is None else int(width)
        h = int(_host(params['org_height'])) if height is None else int(height)
        T = int(params['cam_unnorm_rots'].shape[-1]) if num_frames is None else int(num_frames)
        if first_frame_w2c is None:
            first_frame_w2c = params['w2c'] if 'w2c' in params else np.eye(4)
        first = np.asarray(_host(first_frame_w2c), dtype=np.float32)
        if cam is None:
            cam = setup_camera(w, h, k, first, near, far, device=dev)
        views = run_w2cs(params).cpu().numpy()[:T]
        if not np.array_equal(first, np.eye(4, dtype=np.float32)):
            views = np.stack([first @ m for m in views])
        steps = list(range(0, T, int(every)))
    if cull:
        depths = []
        with torch.no_grad():
            for t in steps:
                _rv, _im, _radius, _sem, depth, opac = slam.render_params(params, t, cam, False)
                depths.append(torch.where(opac > sil_thres, depth, torch.zeros_like(depth)).reshape(h, w).contiguous())
        seen = seen_vertices(gv, views[steps], k, h, w, depths=depths, eps=threshold)
        gv, gf, gl = cull_mesh(gv, gf, seen, gl)
        counts.update(gt_vertices_seen=int(gv.shape[0]), gt_faces_kept=int(gf.shape[0]))
        if gf.shape[0] == 0:
            raise ValueError("hsr_utils.mesh_eval: the cameras saw no face of %s" % gt_ply)
    rec = _mesh(rec_v, rec_f, rec_l if use_labels else None, device=dev)
    aligned = {}
    if align is not None:
        from . import mesh_align
        if align == "icp":
            moved, icp = mesh_align.align_mesh(rec, (gv, gf), n_samples=n_samples, seed=seed, max_dist=align_max_dist,
                                               max_iterations=align_iterations)
            transform = icp["transform"]
            aligned.update(align_fitness=icp["fitness"], align_rmse=icp["inlier_rmse"], align_iterations=icp["iterations"])
        else:
            transform = mesh_align.trajectory_alignment(gt_w2cs, views)
            moved = mesh_align.transform_points(rec[0], transform)
        rec = (moved,) + tuple(rec[1:])
        aligned.update(align=align, align_transform=transform.tolist())
    out = mesh_metrics(rec, (gv, gf, gl), n_samples=n_samples, threshold=threshold, seed=seed, num_classes=num_classes)
    out.update(counts)
    out.update(aligned)
    if depth_views:
        from . import mesh_depth
        from .camera import scale_intrinsics
        dh, dw = (h, w) if depth_size is None else (int(depth_size[0]), int(depth_size[1]))
        dk = scale_intrinsics(k, dh / h, dw / w)
        virtual = mesh_depth.virtual_views(views[steps], gv, depth_views, depth_seed)
        l1 = mesh_depth.mesh_depth_l1(rec[:2], (gv, gf), virtual, dk, dh, dw, near=near)
        out.update(depth_l1=l1["depth_l1"], depth_l1_covered=l1["depth_l1_covered"], depth_gt_cover=l1["gt_cover"],
                   depth_rec_cover=l1["rec_cover"], depth_views=depth_views)
    return out


__all__ = ["face_areas", "sample_mesh", "NearestGrid", "seen_vertices", "cull_mesh", "distance_metrics", "label_metrics", "mesh_metrics",
           "evaluate_mesh_run"]
