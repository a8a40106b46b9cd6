"""Per-frame evaluation of a finished map with the reference's metrics, on the GPU (include/hsr_eval.h); the trajectory error on the host.

    frame_metrics(im, gt_im, depth, gt_depth, final_opacity=None, sil_thres=None)   psnr, depth L1, "depth RMSE"
                                                                                    utils/eval_helpers.py:1258-1295
    semantic_labels(im_semantic, mode, level_sizes=, tree_table=, mlp=)            argmax(softmax): flat :974-983, tree :187-204 +
                                                                                    :135-156, leaf MLP :1251-1255
    tree_levels(level_sizes)                                                       the one check of a level_sizes list: (sizes, tuples)
    tree_lookup_table(label_mapping_tree, level_sizes)                             the dict of transfer_tree_2_label as a dense table
    iou_counts(pred, gt, num_classes=, class_ids=, dilation_ratio=0.02)            calculate_iou :83-90, boundary_iou :37-81, per class
    ms_ssim(im, gt_im, gt_depth, final_opacity=None, sil_thres=None, details=False) MS-SSIM :722, :946, :1272; restated, not pinned
                                                                                    by the reference's package (include/ext/hsr_msssim.h)
    frame_miou(counts)                                                             mean IoU / boundary IoU of a frame :1487-1498
    evaluate_frame(...)                                                            the per-frame body of eval_semantic_tree_newrender
    trajectory_ate(gt_w2c_list, est_w2c_list)                                      evaluate_ate + align :218-275, :1555-1577 (numpy)
    evaluate_sequence(params, frames, cam, eval_dir, ...)                          the loop of eval_semantic_tree_newrender / eval_newrender:
                                                                                    scores per frame, the txt files, the pictures
                                                                                    (hsr_utils.export, include/ext/hsr_frame_export.h)
    view_holes(final_opacity, gt_depth, sil_thres)                                 the hole count of a novel view :1726-1734
                                                                                    (include/ext/hsr_view.h)
    view_percent_holes(holes, numel)                                               percent_holes and the validity rule :1734-1738 (host)
    evaluate_novel_views(params, frames, cam, eval_dir, ...)                       the loop of eval_nvs :1648-1863: the map rendered from
                                                                                    given poses, scored over the valid views

Every per-frame call runs on the current stream and returns device tensors without a host synchronisation: score all frames, read
the numbers once at the end.  Frame averages are plain means over frames (:1590-1600).  There is no CPU path.
"""
import ctypes as C
import math

import numpy as np
import torch

from diff_gaussian_rasterization import _abi

_lib = _abi.lib

MAX_CLASSES, MAX_LEVELS, LEAF_MAX_K, LEAF_MAX_C, MAX_DILATION = 4096, 16, 32, 256, 1024
MSSSIM_SCALES, MSSSIM_MIN_SIDE, MSSSIM_OUT = 5, 161, 31
_class_cache = {}


def _dev(t, what, dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError("hsr_utils.evaluate: %s must be a torch tensor" % what)
    if not t.is_cuda:
        raise RuntimeError("hsr_utils.evaluate: %s must live on a HIP device (got %s); there is no CPU path" % (what, t.device))
    if t.dtype != dtype:
        raise RuntimeError("hsr_utils.evaluate: %s must be %s (got %s)" % (what, dtype, t.dtype))
    return t.contiguous()


def _plane(t, what, H, W, dtype=torch.float32):
    t = _dev(t, what, dtype)
    if t.numel() != H * W or t.shape[-2:] != (H, W):
        raise RuntimeError("hsr_utils.evaluate: %s must be [H,W] or [1,H,W] with H=%d W=%d (got %s)" % (what, H, W, tuple(t.shape)))
    return t


def frame_metrics(im, gt_im, depth, gt_depth, final_opacity=None, sil_thres=None):
    """float64 [3] on the device: psnr, depth_l1, depth_rmse of one frame (utils/eval_helpers.py:1258-1295).  im / gt_im: [3,H,W];
    depth / gt_depth / final_opacity: [1,H,W] or [H,W], all float32.  With final_opacity and sil_thres (the reference's
    `mapping_iters == 0 and not add_new_gaussians` branch) the silhouette mask multiplies the image and depth terms; otherwise only
    gt_depth > 0 does.  PSNR is calc_psnr over all H*W pixels (masked ones as zeros), averaged over the channels; the "RMSE" is the
    reference's mean of sqrt(e^2).  An exact image gives +inf, a frame without valid depth NaN."""
    a = _dev(im, "im")
    if a.dim() != 3 or a.shape[0] != 3:
        raise RuntimeError("hsr_utils.evaluate: im must be [3,H,W] (got %s)" % (tuple(im.shape),))
    H, W = a.shape[1:]
    b = _dev(gt_im, "gt_im")
    if b.shape != a.shape:
        raise RuntimeError("hsr_utils.evaluate: gt_im %s differs from im %s" % (tuple(b.shape), tuple(a.shape)))
    d, gd = _plane(depth, "depth", H, W), _plane(gt_depth, "gt_depth", H, W)
    if (final_opacity is None) != (sil_thres is None):
        raise RuntimeError("hsr_utils.evaluate: final_opacity and sil_thres go together")
    op = None if final_opacity is None else _plane(final_opacity, "final_opacity", H, W)
    dev = a.device
    out = torch.empty(3, dtype=torch.float64, device=dev)
    sc = torch.empty(int(_lib.hsr_eval_metrics_scratch_bytes(H, W)), dtype=torch.uint8, device=dev)
    _abi.call(_lib.hsr_eval_frame_metrics, "hsr_eval_frame_metrics", dev, H, W, a.data_ptr(), b.data_ptr(), d.data_ptr(), gd.data_ptr(),
              None if op is None else op.data_ptr(), 0.0 if sil_thres is None else float(sil_thres), out.data_ptr(), sc.data_ptr(), sc.numel())
    return out


def ms_ssim(im, gt_im, gt_depth, final_opacity=None, sil_thres=None, details=False):
    """0-dim float64 device tensor: the multi-scale SSIM of one frame as the reference scores it (utils/eval_helpers.py:1259-1272:
    ms_ssim(data_range=1.0, size_average=True) of the two images after both were multiplied by gt_depth > 0 and, with final_opacity
    and sil_thres, by the silhouette mask).  Five scales of a valid 11-tap Gaussian filter (sigma 1.5) with 2x2 average pools
    between them, weights 0.0448, 0.2856, 0.3001, 0.2363, 0.1333; include/ext/hsr_msssim.h states every step.  Restated from the
    definition, not pinned by the reference's package (pytorch_msssim).  im / gt_im: [3,H,W]; gt_depth / final_opacity: [1,H,W] or
    [H,W], all float32; min(H, W) > 160.  details=True also returns the float64 [5,3,2] table of the per-scale, per-channel means of
    cs and ssim before the relu.  No host synchronisation, no copy of the images."""
    a = _dev(im, "im")
    if a.dim() != 3 or a.shape[0] != 3:
        raise RuntimeError("hsr_utils.evaluate: im must be [3,H,W] (got %s)" % (tuple(im.shape),))
    H, W = a.shape[1:]
    b = _dev(gt_im, "gt_im")
    if b.shape != a.shape:
        raise RuntimeError("hsr_utils.evaluate: gt_im %s differs from im %s" % (tuple(b.shape), tuple(a.shape)))
    gd = _plane(gt_depth, "gt_depth", H, W)
    if (final_opacity is None) != (sil_thres is None):
        raise RuntimeError("hsr_utils.evaluate: final_opacity and sil_thres go together")
    op = None if final_opacity is None else _plane(final_opacity, "final_opacity", H, W)
    if min(H, W) < MSSSIM_MIN_SIDE:
        raise AssertionError("hsr_utils.evaluate: ms_ssim needs an image whose smaller side is larger than %d, for the 4 downsamplings "
                             "of an 11-tap window (got H=%d W=%d)" % (MSSSIM_MIN_SIDE - 1, H, W))
    dev = a.device
    out = torch.empty(MSSSIM_OUT, dtype=torch.float64, device=dev)
    sc = torch.empty(int(_lib.hsr_eval_msssim_scratch_bytes(H, W)), dtype=torch.uint8, device=dev)
    _abi.call(_lib.hsr_eval_msssim, "hsr_eval_msssim", dev, H, W, a.data_ptr(), b.data_ptr(), gd.data_ptr(),
              None if op is None else op.data_ptr(), 0.0 if sil_thres is None else float(sil_thres), out.data_ptr(), sc.data_ptr(), sc.numel())
    return (out[0], out[1:].view(MSSSIM_SCALES, 3, 2)) if details else out[0]


_ms_ssim = ms_ssim      # evaluate_frame's flag carries the function's name


def tree_levels(level_sizes):
    """(sizes, n): the level sizes of the dataset's num_semantic — level_sizes without its last entry, the leaf count — and the
    number n = prod(sizes) of label tuples, the rows of a table over the mixed-radix tuple index.  The one check of a level_sizes
    list for every function of hsr_utils that takes one: 1..MAX_LEVELS levels of at least one class, at most 2^26 tuples."""
    sizes = [int(s) for s in level_sizes][:-1]
    if not 1 <= len(sizes) <= MAX_LEVELS or min(sizes) < 1:
        raise RuntimeError("hsr_utils.evaluate: level_sizes must list 1..%d level sizes >= 1 plus the leaf count" % MAX_LEVELS)
    n = math.prod(sizes)
    if n > 1 << 26:
        raise RuntimeError("hsr_utils.evaluate: a %d-entry table of the level tuples is too large" % n)
    return sizes, n


def tree_lookup_table(label_mapping_tree, level_sizes, device="cuda"):
    """The dataset's label_mapping_tree ({leaf id (int or str): tuple of per-level labels}) as a dense int32 table over the mixed-radix
    index of the level labels (level 0 most significant), for the levels level_sizes[:-1] (the dataset's num_semantic, whose last
    entry is the leaf count; datasets/gradslam_datasets/replica.py:144-147).  A tuple not in the dict maps to -1; of two keys with one
    tuple the later entry wins, as transfer_tree_2_label's loop of masked assignments does (utils/eval_helpers.py:135-156).  Tuples
    with a label outside its level's range are never produced by the argmax and are left out.  Built once on the host."""
    sizes, n = tree_levels(level_sizes)
    table = np.full(n, -1, dtype=np.int64)
    for key, value in label_mapping_tree.items():
        value = [int(v) for v in value]
        if len(value) != len(sizes):
            raise RuntimeError("hsr_utils.evaluate: tree entry %r has %d levels, level_sizes %d" % (key, len(value), len(sizes)))
        if any(v < 0 or v >= s for v, s in zip(value, sizes)):
            continue
        idx = 0
        for v, s in zip(value, sizes):
            idx = idx * s + v
        table[idx] = int(key)
    if table.min() < -(1 << 31) or table.max() >= 1 << 31:
        raise RuntimeError("hsr_utils.evaluate: leaf ids must fit in int32")
    return torch.tensor(table.astype(np.int32), device=device)


def semantic_labels(im_semantic, mode, *, level_sizes=None, tree_table=None, mlp=None):
    """int32 [H,W] labels argmax(softmax(.)) of the rendered semantic map im_semantic ([K,H,W] float32).
      mode "flat": over all K planes (utils/eval_helpers.py:974-983);
      mode "tree": per level over the channel ranges level_sizes[:-1] (transfer_tree_label, :187-204), then the leaf id of the tuple of
                   level labels from tree_table (tree_lookup_table; -1 where the tuple names no leaf).  Returns (labels, level labels
                   int32 [L,H,W]);
      mode "leaf": over the C logits of the 1x1-conv leaf head `mlp` (a Conv2d(K, C, 1) or a (weight, bias) pair; :1251-1255), which
                   are never materialised.
    Ties are among the fp32 probabilities expf(x_i - max) / sum and go to the lowest index, like torch.argmax."""
    z = _dev(im_semantic, "im_semantic")
    if z.dim() == 4 and z.shape[0] == 1:
        z = z[0]
    if z.dim() != 3:
        raise RuntimeError("hsr_utils.evaluate: im_semantic must be [K,H,W] (got %s)" % (tuple(im_semantic.shape),))
    K, H, W = z.shape
    dev = z.device
    out = torch.empty((H, W), dtype=torch.int32, device=dev)
    if mode == "flat":
        _abi.call(_lib.hsr_eval_labels_flat, "hsr_eval_labels_flat", dev, K, H, W, z.data_ptr(), out.data_ptr())
        return out
    if mode == "tree":
        if level_sizes is None or tree_table is None:
            raise RuntimeError("hsr_utils.evaluate: mode 'tree' needs level_sizes and tree_table")
        sizes, n = tree_levels(level_sizes)
        L = len(sizes)
        if sum(sizes) > K:
            raise RuntimeError("hsr_utils.evaluate: level_sizes %s (levels + leaf count) do not fit %d planes" % (list(level_sizes), K))
        table = _dev(tree_table, "tree_table", torch.int32)
        if table.numel() != n:
            raise RuntimeError("hsr_utils.evaluate: tree_table has %d entries, the levels %s need %d" % (table.numel(), sizes, n))
        levels = torch.empty((L, H, W), dtype=torch.int32, device=dev)
        _abi.call(_lib.hsr_eval_labels_tree, "hsr_eval_labels_tree", dev, K, H, W, L, (C.c_int * L)(*sizes), z.data_ptr(), table.data_ptr(),
                  out.data_ptr(), levels.data_ptr())
        return out, levels
    if mode == "leaf":
        if mlp is None:
            raise RuntimeError("hsr_utils.evaluate: mode 'leaf' needs mlp")
        weight, bias = (mlp.weight, mlp.bias) if hasattr(mlp, "weight") else mlp
        w = _dev(weight.detach(), "mlp weight").reshape(weight.shape[0], -1)
        b = _dev(bias.detach(), "mlp bias").reshape(-1)
        Cc = w.shape[0]
        if w.shape[1] != K or b.numel() != Cc:
            raise RuntimeError("hsr_utils.evaluate: mlp weight %s / bias %s do not match %d planes" % (tuple(weight.shape), tuple(bias.shape), K))
        if K > LEAF_MAX_K or Cc > LEAF_MAX_C:
            raise RuntimeError("hsr_utils.evaluate: the leaf head takes K <= %d planes and C <= %d classes (got K=%d C=%d)"
                               % (LEAF_MAX_K, LEAF_MAX_C, K, Cc))
        sc = torch.empty(int(_lib.hsr_eval_leaf_scratch_bytes(Cc)), dtype=torch.uint8, device=dev)
        _abi.call(_lib.hsr_eval_labels_leaf, "hsr_eval_labels_leaf", dev, K, Cc, H, W, z.data_ptr(), w.contiguous().data_ptr(), b.data_ptr(),
                  out.data_ptr(), sc.data_ptr(), sc.numel())
        return out
    raise RuntimeError("hsr_utils.evaluate: mode must be 'flat', 'tree' or 'leaf' (got %r)" % (mode,))


def dilation_pixels(H, W, dilation_ratio=0.02):
    """mask_to_boundary's erosion count: max(1, int(round(ratio * sqrt(H^2 + W^2)))), round half to even (utils/eval_helpers.py:44-48)."""
    return max(1, int(round(dilation_ratio * float(np.sqrt(H ** 2 + W ** 2)))))


def _classes(class_ids, dev):
    key = (tuple(int(c) for c in class_ids), dev)
    if key not in _class_cache:
        ids = np.asarray(key[0], dtype=np.int64)
        if len(np.unique(ids)) != len(ids):
            raise RuntimeError("hsr_utils.evaluate: class_ids must be distinct")
        if ids.size and (ids.min() < -(1 << 31) or ids.max() >= 1 << 31):
            raise RuntimeError("hsr_utils.evaluate: class_ids must fit in int32")
        order = np.argsort(ids, kind="stable")
        _class_cache[key] = (torch.tensor(ids[order].astype(np.int32), device=dev), torch.tensor(order.astype(np.int32), device=dev))
    return _class_cache[key]


def iou_counts(pred, gt, num_classes=None, class_ids=None, dilation_ratio=0.02):
    """int64 [C,6] on the device, per class c: [G, P, I, G_b, P_b, I_b] with G = |gt == c|, P = |pred == c|, I = |both|, and the same
    over the boundary pixels of mask_to_boundary (utils/eval_helpers.py:37-90); the union is G + P - I.  pred / gt: int32 label maps
    [H,W].  Classes: range(num_classes), or the labels of class_ids (distinct ints, any order; rows follow it) as the ScanNet
    tree_large branch iterates dataset.semantic_id (:1407).  A label in neither set counts for no class.  C <= 4096."""
    p = _dev(pred, "pred", torch.int32)
    H, W = p.shape[-2:]
    p = _plane(p, "pred", H, W, torch.int32)
    g = _plane(gt, "gt", H, W, torch.int32)
    if (num_classes is None) == (class_ids is None):
        raise RuntimeError("hsr_utils.evaluate: give exactly one of num_classes and class_ids")
    Cc = int(num_classes) if class_ids is None else len(class_ids)
    if not 1 <= Cc <= MAX_CLASSES:
        raise RuntimeError("hsr_utils.evaluate: %d classes; 1..%d are supported" % (Cc, MAX_CLASSES))
    d = dilation_pixels(H, W, dilation_ratio)
    if d > MAX_DILATION:
        raise RuntimeError("hsr_utils.evaluate: a boundary width of %d pixels exceeds %d" % (d, MAX_DILATION))
    dev = p.device
    ids = rows = None
    if class_ids is not None:
        ids, rows = _classes(class_ids, dev)
    out = torch.empty((Cc, 6), dtype=torch.int64, device=dev)
    sc = torch.empty(int(_lib.hsr_eval_iou_scratch_bytes(H, W)), dtype=torch.uint8, device=dev)
    _abi.call(_lib.hsr_eval_iou_counts, "hsr_eval_iou_counts", dev, H, W, p.data_ptr(), g.data_ptr(), Cc,
              None if ids is None else ids.data_ptr(), None if rows is None else rows.data_ptr(), d, out.data_ptr(), sc.data_ptr(), sc.numel())
    return out


def frame_miou(counts):
    """float64 [2] on the device: the frame's mean IoU and mean boundary IoU over the classes with G + P > 0
    (utils/eval_helpers.py:1487-1498); NaN when no class is present, like np.mean([])."""
    q = _dev(counts, "counts", torch.int64)
    if q.dim() != 2 or q.shape[1] != 6:
        raise RuntimeError("hsr_utils.evaluate: counts must be [C,6] (got %s)" % (tuple(q.shape),))
    out = torch.empty(2, dtype=torch.float64, device=q.device)
    _abi.call(_lib.hsr_eval_frame_miou, "hsr_eval_frame_miou", q.device, q.shape[0], q.data_ptr(), out.data_ptr())
    return out


def evaluate_frame(im, gt_im, depth, gt_depth, im_semantic, gt_labels, mode, *, final_opacity=None, sil_thres=None, level_sizes=None,
                   tree_table=None, mlp=None, num_classes=None, class_ids=None, dilation_ratio=0.02, ms_ssim=False):
    """The per-frame scores of eval_semantic_tree_newrender (utils/eval_helpers.py:1258-1498) without MS-SSIM and LPIPS: a dict of
    0-dim device tensors psnr, depth_l1, depth_rmse (float64), miou, mbiou (float64).  im / im_semantic / depth / final_opacity as the
    semantic rasterizer returns them; gt_labels: the leaf label map ([H,W], int; label_gt[-1] for tree datasets).  `mode` and its
    arguments as semantic_labels; num_classes / class_ids as iou_counts.  With ms_ssim=True the dict is without LPIPS only: it gains
    the key ms_ssim (float64, the function ms_ssim of this module on the same images and masks).  No host synchronisation."""
    return _frame_scores(im, gt_im, depth, gt_depth, im_semantic, gt_labels, mode, final_opacity, sil_thres, level_sizes, tree_table, mlp,
                         num_classes, class_ids, dilation_ratio, ms_ssim)[0]


def _frame_scores(im, gt_im, depth, gt_depth, im_semantic, gt_labels, mode, final_opacity, sil_thres, level_sizes, tree_table, mlp,
                  num_classes, class_ids, dilation_ratio, ms_ssim):
    """evaluate_frame's body: (its dict, the predicted int32 [H,W] label map, which evaluate_sequence's pictures reuse)"""
    m = frame_metrics(im, gt_im, depth, gt_depth, final_opacity, sil_thres)
    lab = semantic_labels(im_semantic, mode, level_sizes=level_sizes, tree_table=tree_table, mlp=mlp)
    if mode == "tree":
        lab = lab[0]
    H, W = lab.shape
    g = gt_labels.reshape(H, W)
    if g.dtype != torch.int32:
        g = g.to(torch.int32)
    s = frame_miou(iou_counts(lab, g, num_classes=num_classes, class_ids=class_ids, dilation_ratio=dilation_ratio))
    scores = {"psnr": m[0], "depth_l1": m[1], "depth_rmse": m[2], "miou": s[0], "mbiou": s[1]}
    if ms_ssim:
        scores["ms_ssim"] = _ms_ssim(im, gt_im, gt_depth, final_opacity, sil_thres)
    return scores, lab


def _align(model, data):
    """align() of utils/eval_helpers.py:218-256 (Horn, closed form) without np.matrix: model, data 3 x n; returns rot, trans, errors."""
    mu_m, mu_d = model.mean(1).reshape(3, 1), data.mean(1).reshape(3, 1)
    Wm = (model - mu_m) @ (data - mu_d).T
    U, _d, Vh = np.linalg.svd(Wm.T)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vh) < 0:
        S[2, 2] = -1
    rot = U @ S @ Vh
    trans = mu_d - rot @ mu_m
    err = rot @ model + trans - data
    return rot, trans, np.sqrt(np.sum(err * err, 0))


def _np(m):
    return m.detach().cpu().double().numpy() if isinstance(m, torch.Tensor) else np.asarray(m, dtype=np.float64)


def trajectory_ate(gt_w2c_list, est_w2c_list, first_frame_w2c=None):
    """Average translational error after Horn alignment, as eval_semantic_tree_newrender computes it (utils/eval_helpers.py:1555-1577
    with evaluate_ate / align, :218-275): the [:3,3] columns of the world-to-camera matrices are aligned (not camera centres), frames
    whose gt pose holds a NaN are skipped, and frame 0's estimate is first_frame_w2c (default: gt_w2c_list[0], which is what the
    reference's first_frame_w2c = inv(pose_0) equals).  Lists of 4x4 tensors or arrays, one per frame of the estimate.  Host numpy."""
    n = len(est_w2c_list)
    if n < 1 or len(gt_w2c_list) < n:
        raise RuntimeError("hsr_utils.evaluate: %d estimated poses for %d gt poses" % (n, len(gt_w2c_list)))
    gts = [_np(gt_w2c_list[0])]
    ests = [_np(gt_w2c_list[0] if first_frame_w2c is None else first_frame_w2c)]
    for i in range(1, n):
        g = _np(gt_w2c_list[i])
        if np.isnan(g).any():
            continue
        gts.append(g)
        ests.append(_np(est_w2c_list[i]))
    gt_pts = np.stack([m[:3, 3] for m in gts]).T
    est_pts = np.stack([m[:3, 3] for m in ests]).T
    _rot, _trans, err = _align(gt_pts, est_pts)
    return float(err.mean())


SEQUENCE_FILES = {"psnr": "psnr.txt", "depth_rmse": "rmse.txt", "depth_l1": "l1.txt", "ms_ssim": "ssim.txt", "miou": "miou.txt",
                  "mbiou": "mbiou.txt"}


def evaluate_sequence(params, frames, cam, eval_dir=None, *, eval_every=1, sil_thres, mapping_iters, add_new_gaussians, mode,
                      save_frames=False, level_sizes=None, tree_table=None, mlp=None, num_classes=None, class_ids=None,
                      dilation_ratio=0.02, tuple_table=None, label_table=None, depth_table=None, depth_range=(0.0, 6.0), ms_ssim=True):
    """The loop of eval_semantic_tree_newrender (utils/eval_helpers.py:1145-1646; scripts/hierslam.py:2181-2230) over a finished map:
    with mode=None, and then without semantic planes, scores or pictures, the loop of eval_newrender (:645-).

    params: the final map and poses (SlamSession.params, or map_io's).  frames: any iterable of the session's frame dicts ('id', 'im',
    'depth', optional 'gt_w2c' and 'semantic_label_gt' [levels + 1 leaf, H, W]), read once and in order, so a generator over
    session.ingest(...) works.  cam: the camera of the frames' size.  Every frame's gt pose is kept for the ATE; a frame is rendered
    and scored when its id is 0 or (id + 1) % eval_every == 0 (:1233).  It is rendered from `params` at its estimated pose as
    SlamSession.render does (slam.render_params) and scored by evaluate_frame with mode, level_sizes, tree_table, mlp, num_classes,
    class_ids and dilation_ratio as there; the silhouette mask (final opacity > sil_thres) enters the scores when mapping_iters == 0
    and not add_new_gaussians (:1264-1275).  With mode=None the scores are frame_metrics' and ms_ssim's alone.

    With save_frames (and eval_dir) one hsr_utils.export.export_frame launch per scored frame makes all of the frame's pictures, written
    under the reference's names: rendered_rgb/gs_%04d.png, rendered_depth/gs_%04d.png, rgb/gt_%04d.png, depth/gt_%04d.png (depth_table,
    depth_range as export_frame's) and, with a mode, rendered_semantic/sem_%04d_multilevel.png (mode "tree": the rendered map's level
    labels coloured by tuple_table) or rendered_semantic/sem_%04d.png (modes "leaf" and "flat": the predicted classes coloured by
    label_table) and rendered_semantic/gt_%04d.png (the ground-truth level planes by tuple_table where it is given, else the
    ground-truth classes by label_table).  A saved picture costs one device-to-host copy.

    The scores stay on the device and are read once after the last frame.  With eval_dir: psnr.txt, rmse.txt, l1.txt, ssim.txt (with
    ms_ssim), miou.txt and mbiou.txt (with a mode) via np.savetxt, one row per scored frame, and summary.txt with the reference's
    summary line.  Returns a dict: 'frame_ids', the lists 'psnr', 'depth_l1', 'depth_rmse', 'ms_ssim', 'miou', 'mbiou' (float64 arrays)
    and their plain means 'avg_psnr', ... (:1587-1600), and 'ate_rmse' (trajectory_ate over the frames read, :1554-1584; None when no
    frame carries a gt pose).

    Not built: LPIPS (no weights here; lpips.txt is left out), the matplotlib plots, wandb, and the gt_transfer branch."""
    import os
    from . import slam
    if save_frames and eval_dir is None:
        raise RuntimeError("hsr_utils.evaluate: save_frames needs eval_dir")
    if int(eval_every) < 1:
        raise ValueError("hsr_utils.evaluate: eval_every must be >= 1, not %r" % (eval_every,))
    if mode not in (None, "flat", "tree", "leaf"):
        raise RuntimeError("hsr_utils.evaluate: mode must be None, 'flat', 'tree' or 'leaf' (got %r)" % (mode,))
    use_sil = int(mapping_iters) == 0 and not add_new_gaussians
    dirs = {}
    if eval_dir is not None:
        os.makedirs(eval_dir, exist_ok=True)
    if save_frames:
        from . import export
        for name in ("rendered_rgb", "rendered_depth", "rgb", "depth") + (("rendered_semantic",) if mode is not None else ()):
            dirs[name] = os.path.join(eval_dir, name)
            os.makedirs(dirs[name], exist_ok=True)
    gt_w2c_list, ids, rows = [], [], []
    for frame in frames:
        time_idx = int(frame['id'])
        gt_w2c_list.append(frame.get('gt_w2c'))
        if time_idx != 0 and (time_idx + 1) % int(eval_every) != 0:
            continue
        with torch.no_grad():
            _rv, im, _radius, sem, depth, opac = slam.render_params(params, time_idx, cam, mode is not None)
        op, thres = (opac, sil_thres) if use_sil else (None, None)
        lab = label_gt = None
        if mode is None:
            m = frame_metrics(im, frame['im'], depth, frame['depth'], op, thres)
            scores = {"psnr": m[0], "depth_l1": m[1], "depth_rmse": m[2]}
            if ms_ssim:
                scores["ms_ssim"] = _ms_ssim(im, frame['im'], frame['depth'], op, thres)
        else:
            label_gt = frame['semantic_label_gt']
            scores, lab = _frame_scores(im, frame['im'], depth, frame['depth'], sem, label_gt[-1], mode, op, thres, level_sizes, tree_table,
                                        mlp, num_classes, class_ids, dilation_ratio, ms_ssim)
        ids.append(time_idx)
        rows.append(scores)
        if save_frames:
            want = dict(im=im, gt_im=frame['im'], depth=depth, gt_depth=frame['depth'])
            names = dict(im=("rendered_rgb", "gs_%04d.png"), depth=("rendered_depth", "gs_%04d.png"), gt_im=("rgb", "gt_%04d.png"),
                         gt_depth=("depth", "gt_%04d.png"))
            if mode == "tree":
                want["im_semantic"] = sem
                names["im_semantic"] = ("rendered_semantic", "sem_%04d_multilevel.png")
            elif mode is not None:
                want["labels"] = lab
                names["labels"] = ("rendered_semantic", "sem_%04d.png")
            if mode is not None:
                if tuple_table is not None:
                    gl = label_gt[:-1]
                    want["gt_levels"] = gl if gl.dtype == torch.int64 else gl.to(torch.int64)
                    names["gt_levels"] = ("rendered_semantic", "gt_%04d.png")
                else:
                    want["gt_labels"] = label_gt[-1]
                    names["gt_labels"] = ("rendered_semantic", "gt_%04d.png")
            pictures = export.export_frame(depth_table=depth_table, depth_range=depth_range, level_sizes=level_sizes, tuple_table=tuple_table,
                                           label_table=label_table, **want)
            for key, (sub, pattern) in names.items():
                export.write_png(os.path.join(dirs[sub], pattern % time_idx), pictures[key])
    if not rows:
        raise RuntimeError("hsr_utils.evaluate: evaluate_sequence got no frame to score")
    keys = [k for k in SEQUENCE_FILES if k in rows[0]]
    table = torch.stack([torch.stack([r[k].to(torch.float64) for k in keys]) for r in rows]).cpu().numpy()      # the one read
    result = {"frame_ids": ids}
    for col, k in enumerate(keys):
        result[k] = table[:, col].copy()
        result["avg_" + k] = float(result[k].mean())
    n = min(len(gt_w2c_list), int(params['cam_unnorm_rots'].shape[-1]))
    result["ate_rmse"] = None
    if gt_w2c_list[0] is not None and all(g is not None for g in gt_w2c_list[:n]):
        result["ate_rmse"] = trajectory_ate(gt_w2c_list[:n], [slam.frame_w2c(params, t) for t in range(n)])
    if eval_dir is not None:
        for k in keys:
            np.savetxt(os.path.join(eval_dir, SEQUENCE_FILES[k]), result[k])
        cols = [("ATE RMSE", None if result["ate_rmse"] is None else result["ate_rmse"] * 100)] + [
            (title, result["avg_" + k] * scale) for k, title, scale in (
                ("psnr", "PSNR", 1.0), ("ms_ssim", "MS-SSIM", 1.0), ("depth_l1", "Depth L1", 100.0), ("depth_rmse", "Depth RMSE", 100.0),
                ("miou", "miou%", 100.0), ("mbiou", "mbiou%", 100.0)) if k in keys]
        with open(os.path.join(eval_dir, "summary.txt"), "w") as f:
            f.write(" ".join("[%s]" % title for title, _v in cols) + "\n")
            f.write("\t".join("nan" if v is None else "%.3f" % v for _t, v in cols) + "\n")
    return result


# ---- novel views -------------------------------------------------------------------------------------------------------------------------
VALID_MAX_PERCENT_HOLES = np.float32(0.1)      # utils/eval_helpers.py:1735, the Python 0.1 beside a float32 tensor


def view_holes(final_opacity, gt_depth, sil_thres):
    """int64 [2] on the device: [the pixels with !(final_opacity > sil_thres) and gt_depth > 0, the pixels with gt_depth > 0] of one
    rendered view — the ~(presence_sil_mask | ~valid_depth_mask).sum() of eval_nvs (utils/eval_helpers.py:1726-1734) and the number of
    valid-depth pixels.  A NaN opacity is a hole.  final_opacity / gt_depth: [1,H,W] or [H,W], float32.  Two small launches
    (hsr_view_holes), no host synchronisation: count every view, read once."""
    op = _dev(final_opacity, "final_opacity")
    if op.dim() < 2:
        raise RuntimeError("hsr_utils.evaluate: final_opacity must be [H,W] or [1,H,W] (got %s)" % (tuple(op.shape),))
    H, W = (int(v) for v in op.shape[-2:])
    op, gd = _plane(op, "final_opacity", H, W), _plane(gt_depth, "gt_depth", H, W)
    dev = op.device
    out = torch.empty(2, dtype=torch.int64, device=dev)
    sc = torch.empty(int(_lib.hsr_view_holes_scratch_bytes(H, W)), dtype=torch.uint8, device=dev)
    _abi.call(_lib.hsr_view_holes, "hsr_view_holes", dev, H, W, op.data_ptr(), gd.data_ptr(), float(sil_thres), out.data_ptr(), sc.data_ptr(),
              sc.numel())
    return out


def view_percent_holes(holes, numel):
    """(percent_holes float32, valid bool) from integer hole counts (an int or an integer array) and the pixel count of the frame, as
    torch evaluates eval_nvs's `(~m).sum() / m.numel() * 100 > 0.1` (utils/eval_helpers.py:1734-1738): the int64 sum and numel become
    float32, one float32 division, one float32 product with 100, and the comparison against 0.1 rounded to float32.  A view is valid
    when percent_holes <= 0.1.  Host numpy."""
    pct = np.asarray(holes, dtype=np.int64).astype(np.float32) / np.float32(numel) * np.float32(100)
    return pct, ~(pct > VALID_MAX_PERCENT_HOLES)


NVS_FILES = {"psnr": "psnr.txt", "depth_rmse": "rmse.txt", "depth_l1": "l1.txt", "ms_ssim": "ssim.txt"}


def evaluate_novel_views(params, frames, cam, eval_dir=None, *, eval_every=1, sil_thres, mapping_iters, add_new_gaussians, save_frames=False,
                         depth_table=None, depth_range=(0.0, 6.0), ms_ssim=True):
    """The loop of eval_nvs (utils/eval_helpers.py:1648-1863; scripts/eval_novel_view.py): the finished map `params` rendered from
    held-out poses and scored against their images.

    frames: what the reference's NVS dataset delivers (hsr_utils.sequence.ReplicaV2Sequence(use_train_split=False) once ingested): any
    iterable of dicts with 'im' [3,H,W], 'depth' [1,H,W] (float32, on the device) and 'gt_w2c' [4,4] relative to the first training
    frame, read once and in order.  The FIRST item is the first training frame and is skipped (:1679-1685); the item at position i >= 1
    is test view test_time_idx = i - 1, scored when test_time_idx == 0 or (test_time_idx + 1) % eval_every == 0 (:1688-1690).  A scored
    view without 'gt_w2c' is a RuntimeError.  cam: the camera of the frames' size (setup_camera on the first frame's pose, :1683).

    Per scored view: one slam.render_view call from gt_w2c with the plain rasterizer, whose depth and final opacity stand for the
    reference's separate depth-and-silhouette render (as in evaluate_sequence); view_holes; frame_metrics and (with ms_ssim) ms_ssim,
    with the silhouette mask only when mapping_iters == 0 and not add_new_gaussians (:1742-1773).  With save_frames (and eval_dir) one
    hsr_utils.export.export_frame launch writes rendered_rgb/render_%04d.png, rendered_depth/render_%04d.png, rgb/gt_%04d.png and
    depth/gt_%04d.png, numbered by test_time_idx (:1786-1796; depth_table, depth_range as export_frame's).

    Scores and counts stay on the device and are read once after the last view.  A view is valid when percent_holes <= 0.1
    (view_percent_holes, :1734-1738).  With eval_dir: psnr.txt, rmse.txt, l1.txt, ssim.txt (with ms_ssim) via np.savetxt, one row per
    scored view, and valid_nvs_frames.npy.  Returns a dict: 'frame_ids' (the test_time_idx of the scored views), the arrays 'psnr',
    'depth_l1', 'depth_rmse', 'ms_ssim' (float64), 'holes' and 'valid_depth' (int64, view_holes' two counts), 'percent_holes' (float32)
    and 'valid_nvs_frames' (bool), and 'avg_psnr', ... the means over the VALID views only (:1820-1824): NaN when none is valid.

    Not built: LPIPS (no weights here; lpips.txt is left out), the per-view plots, metrics.png and wandb."""
    import os
    from . import slam
    if save_frames and eval_dir is None:
        raise RuntimeError("hsr_utils.evaluate: save_frames needs eval_dir")
    if int(eval_every) < 1:
        raise ValueError("hsr_utils.evaluate: eval_every must be >= 1, not %r" % (eval_every,))
    use_sil = int(mapping_iters) == 0 and not add_new_gaussians
    dirs = {}
    if eval_dir is not None:
        os.makedirs(eval_dir, exist_ok=True)
    if save_frames:
        from . import export
        for name in ("rendered_rgb", "rendered_depth", "rgb", "depth"):
            dirs[name] = os.path.join(eval_dir, name)
            os.makedirs(dirs[name], exist_ok=True)
    keys = ["psnr", "depth_l1", "depth_rmse"] + (["ms_ssim"] if ms_ssim else [])
    ids, rows, numel = [], [], []
    for position, frame in enumerate(frames):
        if position == 0:      # the first training frame: it fixes the camera in the reference and is not scored
            continue
        test_time_idx = position - 1
        if test_time_idx != 0 and (test_time_idx + 1) % int(eval_every) != 0:
            continue
        if frame.get('gt_w2c') is None:
            raise RuntimeError("hsr_utils.evaluate: novel view %d carries no 'gt_w2c'" % test_time_idx)
        _rv, im, _radius, _sem, depth, opac = slam.render_view(params, frame['gt_w2c'], cam, False)
        holes = view_holes(opac, frame['depth'], sil_thres)
        op, thres = (opac, sil_thres) if use_sil else (None, None)
        scores = list(frame_metrics(im, frame['im'], depth, frame['depth'], op, thres))
        if ms_ssim:
            scores.append(_ms_ssim(im, frame['im'], frame['depth'], op, thres))
        ids.append(test_time_idx)
        numel.append(int(opac.numel()))
        rows.append(torch.cat([torch.stack(scores), holes.to(torch.float64)]))      # counts below 2^31 are exact in float64
        if save_frames:
            pictures = export.export_frame(im=im, gt_im=frame['im'], depth=depth, gt_depth=frame['depth'], depth_table=depth_table,
                                           depth_range=depth_range)
            for key, (sub, pattern) in dict(im=("rendered_rgb", "render_%04d.png"), depth=("rendered_depth", "render_%04d.png"),
                                            gt_im=("rgb", "gt_%04d.png"), gt_depth=("depth", "gt_%04d.png")).items():
                export.write_png(os.path.join(dirs[sub], pattern % test_time_idx), pictures[key])
    if not rows:
        raise RuntimeError("hsr_utils.evaluate: evaluate_novel_views got no view to score")
    table = torch.stack(rows).cpu().numpy()      # the one read
    result = {"frame_ids": ids}
    for col, k in enumerate(keys):
        result[k] = table[:, col].copy()
    result["holes"] = table[:, len(keys)].astype(np.int64)
    result["valid_depth"] = table[:, len(keys) + 1].astype(np.int64)
    result["percent_holes"], valid = view_percent_holes(result["holes"], np.asarray(numel, dtype=np.int64))
    result["valid_nvs_frames"] = valid
    for k in keys:
        result["avg_" + k] = float(result[k][valid].mean()) if valid.any() else float("nan")
    if eval_dir is not None:
        for k in keys:
            np.savetxt(os.path.join(eval_dir, NVS_FILES[k]), result[k])
        np.save(os.path.join(eval_dir, "valid_nvs_frames.npy"), valid)
    return result


__all__ = ["frame_metrics", "ms_ssim", "semantic_labels", "tree_levels", "tree_lookup_table", "iou_counts", "frame_miou", "evaluate_frame", "trajectory_ate",
           "dilation_pixels", "evaluate_sequence", "view_holes", "view_percent_holes", "evaluate_novel_views"]
