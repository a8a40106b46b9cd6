"""Numpy restatement of the reference's per-frame evaluation (utils/eval_helpers.py, eval_semantic_tree_newrender :1184-1630), the
checker of hsr_utils/evaluate.py.  Line numbers cite utils/eval_helpers.py unless another file is named.  Host only.

Boundaries come in three forms that tests/test_eval_cpu.py proves identical:
  boundary_cv2       mask_to_boundary (:37-56) literally: copyMakeBorder(mask, 1, 1, 1, 1, BORDER_CONSTANT, 0), then `d` iterations of a
                     3x3 erosion whose border value does not erode (cv2.erode's default), crop, mask - eroded;
  boundary_scipy     the same with scipy.ndimage.binary_erosion(border_value=1, iterations=d);
  boundary_flags     the form the kernel uses, one flag per pixel for every class: within d-1 rows / columns of the edge, or the
                     (2d+1)^2 window's minimum label differs from its maximum.
"""
import numpy as np


# ---------------------------------------------------------------- frame metrics (:1258-1295, calc_psnr utils/slam_external.py:49-51)
def frame_metrics(im, gt_im, depth, gt_depth, final_opacity=None, sil_thres=None, dtype=np.float64):
    """psnr, depth_l1, depth_rmse; im / gt_im [3,H,W], depth / gt_depth / final_opacity [1,H,W] or [H,W]."""
    im, gt_im = np.asarray(im, dtype), np.asarray(gt_im, dtype)
    H, W = im.shape[1:]
    depth, gt_depth = np.asarray(depth, dtype).reshape(1, H, W), np.asarray(gt_depth, dtype).reshape(1, H, W)
    valid = (gt_depth > 0)                                                  # :1259
    rastered = depth * valid                                                # :1261
    with np.errstate(divide="ignore", invalid="ignore"):
        if final_opacity is not None:                                       # mapping_iters == 0 and not add_new_gaussians
            presence = np.asarray(final_opacity, dtype).reshape(H, W) > sil_thres    # :1262-1263
            w_im, w_gt = im * presence * valid, gt_im * presence * valid     # :1266-1267
            diff = (rastered - gt_depth) * presence                          # :1282, :1285
        else:
            w_im, w_gt = im * valid, gt_im * valid                           # :1269-1270
            diff = rastered - gt_depth                                       # :1288, :1291
        mse = ((w_im - w_gt) ** 2).reshape(3, -1).mean(1)                    # calc_psnr
        psnr = (20 * np.log10(1.0 / np.sqrt(mse))).mean()                    # :1271
        rmse = (np.sqrt(diff ** 2) * valid).sum() / valid.sum()              # :1283-1284 ("RMSE": a mean of |e|)
        l1 = (np.abs(diff) * valid).sum() / valid.sum()                      # :1286-1287
    return np.array([psnr, l1, rmse], dtype=np.float64)


# ---------------------------------------------------------------- labels
def softmax_argmax(x, axis=0):
    """argmax(softmax(x)) with fp32 probabilities expf(x - max) / sum; the first maximum wins (:974-983, :187-204)."""
    x = np.asarray(x, np.float32)
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return np.argmax(e / e.sum(axis=axis, keepdims=True), axis=axis).astype(np.int32)


def tree_level_labels(im_semantic, level_sizes):
    """transfer_tree_label (:187-204): the levels level_sizes[:-1] (the dataset's num_semantic ends with the leaf count)."""
    out, b = [], 0
    for n in list(level_sizes)[:-1]:
        out.append(softmax_argmax(im_semantic[b:b + n]))
        b += n
    return np.stack(out)


def tree_to_leaf(level_labels, label_mapping_tree):
    """transfer_tree_2_label (:135-156): -1 everywhere, then one masked assignment per dict entry in dict order."""
    out = np.full(level_labels.shape[1:], -1, dtype=np.int64)
    for key, value in label_mapping_tree.items():
        idx = np.all(level_labels == np.asarray(value).reshape(-1, 1, 1), axis=0)
        out[idx] = int(key)
    return out


# ---------------------------------------------------------------- boundaries (:37-81)
def dilation_pixels(H, W, dilation_ratio=0.02):
    return max(1, int(round(dilation_ratio * np.sqrt(H ** 2 + W ** 2))))   # :44-48


def boundary_cv2(mask, d):
    """mask_to_boundary for a 0/1 mask: pad by one zero, d erosions of 3x3 (the border outside the padded image does not erode)."""
    m = np.pad(np.asarray(mask, np.uint8), 1, constant_values=0)
    for _ in range(d):
        p = np.pad(m, 1, constant_values=1)
        h, w = m.shape
        m = np.min([p[i:i + h, j:j + w] for i in range(3) for j in range(3)], axis=0)
    return np.asarray(mask, np.uint8) - m[1:-1, 1:-1]


def boundary_scipy(mask, d):
    from scipy import ndimage
    mask = np.asarray(mask, bool)
    er = ndimage.binary_erosion(np.pad(mask, 1), structure=np.ones((3, 3), bool), iterations=d, border_value=1)[1:-1, 1:-1]
    return (mask & ~er).astype(np.uint8)


def _window(a, d, fn, fill):
    """fn over the clipped (2d+1)^2 window, separable: rows then columns."""
    H, W = a.shape
    p = np.pad(a, ((0, 0), (d, d)), constant_values=fill)
    r = fn(np.lib.stride_tricks.sliding_window_view(p, 2 * d + 1, axis=1), axis=-1)
    p = np.pad(r, ((d, d), (0, 0)), constant_values=fill)
    return fn(np.lib.stride_tricks.sliding_window_view(p, 2 * d + 1, axis=0), axis=-1)


def boundary_flags(labels, d):
    """One flag per pixel: on the boundary of its own class (kernel formulation)."""
    lab = np.asarray(labels, np.int64)
    H, W = lab.shape
    big = np.iinfo(np.int64)
    wmin, wmax = _window(lab, d, np.min, big.max), _window(lab, d, np.max, big.min)
    yy, xx = np.mgrid[0:H, 0:W]
    edge = (yy < d) | (yy > H - 1 - d) | (xx < d) | (xx > W - 1 - d)
    return edge | (wmin != wmax)


# ---------------------------------------------------------------- IoU (:83-90, :1297-1498)
def iou_counts(pred, gt, classes, dilation_ratio=0.02):
    """int64 [C,6]: G, P, I, G_b, P_b, I_b per class of `classes` (label values), via boundary_flags."""
    pred, gt = np.asarray(pred, np.int64), np.asarray(gt, np.int64)
    d = dilation_pixels(*gt.shape, dilation_ratio)
    fg, fp = boundary_flags(gt, d), boundary_flags(pred, d)
    C = len(classes)
    row = {int(c): j for j, c in enumerate(classes)}
    jg = np.vectorize(lambda v: row.get(int(v), C), otypes=[np.int64])(gt).ravel()    # C = in no class
    jp = np.vectorize(lambda v: row.get(int(v), C), otypes=[np.int64])(pred).ravel()
    fg, fp = fg.ravel(), fp.ravel()
    both = jg == jp
    cnt = lambda j, w: np.bincount(j, weights=w, minlength=C + 1)[:C].astype(np.int64)
    one = np.ones_like(fg, dtype=np.float64)
    return np.stack([cnt(jg, one), cnt(jp, one), cnt(jg, both * 1.0), cnt(jg, fg * 1.0), cnt(jp, fp * 1.0),
                     cnt(jg, (both & fg & fp) * 1.0)], axis=1)


def frame_miou(counts):
    """[mean IoU, mean boundary IoU] over the classes present (:1487-1498); NaN for none, like np.mean([])."""
    iou, biou = [], []
    for G, P, I, Gb, Pb, Ib in np.asarray(counts, np.int64):
        if G + P == 0:                                                      # :1410-1411, :1446-1447
            continue
        iou.append(I / (G + P - I))                                          # calculate_iou
        biou.append(Ib / (Gb + Pb - Ib))                                     # boundary_iou
    return np.array([np.mean(iou) if iou else np.nan, np.mean(biou) if biou else np.nan])


def frame_miou_literal(pred, gt, classes, dilation_ratio=0.02):
    """The reference's per-class loop as written (calculate_iou, boundary_iou with the cv2 recipe); small maps only."""
    d = dilation_pixels(*np.shape(gt), dilation_ratio)
    iou, biou = [], []
    for c in classes:
        p, g = (np.asarray(pred) == c).astype(np.float32), (np.asarray(gt) == c).astype(np.float32)
        if p.sum() == 0 and g.sum() == 0:
            continue
        iou.append(np.sum(np.logical_and(g > 0, p > 0)) / np.sum(np.logical_or(g > 0, p > 0)))
        gb, pb = boundary_cv2((g > 0).astype(np.uint8), d), boundary_cv2((p > 0).astype(np.uint8), d)
        biou.append(((gb * pb) > 0).sum() / ((gb + pb) > 0).sum())
    return np.array([np.mean(iou) if iou else np.nan, np.mean(biou) if biou else np.nan])


# ---------------------------------------------------------------- ATE (:218-275, :1555-1577)
def align(model, data):
    """align() as written, np.matrix included."""
    model, data = np.asmatrix(model), np.asmatrix(data)
    model_zerocentered = model - model.mean(1).reshape((3, -1))
    data_zerocentered = data - data.mean(1).reshape((3, -1))
    W = np.zeros((3, 3))
    for column in range(model.shape[1]):
        W += np.outer(model_zerocentered[:, column], data_zerocentered[:, column])
    U, d, Vh = np.linalg.svd(W.transpose())
    S = np.matrix(np.identity(3))
    if np.linalg.det(U) * np.linalg.det(Vh) < 0:
        S[2, 2] = -1
    rot = U * S * Vh
    trans = data.mean(1).reshape((3, -1)) - rot * model.mean(1).reshape((3, -1))
    model_aligned = rot * model + trans
    alignment_error = model_aligned - data
    return rot, trans, np.sqrt(np.sum(np.multiply(alignment_error, alignment_error), 0)).A[0]


def trajectory_ate(gt_w2c_list, est_w2c_list):
    """:1555-1577: frame 0's estimate is first_frame_w2c = gt_w2c_list[0]; frames with a NaN gt pose are skipped."""
    gts, ests = [np.asarray(gt_w2c_list[0], np.float64)], [np.asarray(gt_w2c_list[0], np.float64)]
    for i in range(1, len(est_w2c_list)):
        g = np.asarray(gt_w2c_list[i], np.float64)
        if np.isnan(g).sum() > 0:
            continue
        gts.append(g)
        ests.append(np.asarray(est_w2c_list[i], np.float64))
    _, _, err = align(np.stack([m[:3, 3] for m in gts]).T, np.stack([m[:3, 3] for m in ests]).T)
    return float(err.mean())
