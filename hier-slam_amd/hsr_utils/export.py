"""The pictures of one evaluated frame as 8-bit R G B images, on the device (include/ext/hsr_frame_export.h): what
the reference's eval_*_newrender does between the float maps of a frame and cv2.imwrite (utils/eval_helpers.py:1520-1537 for colour and
depth, :1314-1353 with semantic_label_vis / semantic_label_vis_replica :92-133 for the maps coloured per tree tuple, :1054, :1070, :1335
for the maps coloured per class).  The mirror image of hsr_utils.frames: float maps back to 8-bit images.

    jet_colormap(device)                                              the depth pictures' colour table, uint8 [256,3]
    label_colormap(n, device)                                         the per-class colour table, uint8 [n,3]
    tuple_colour_table(colour_map_level, level_sizes, wildcard, device)   the per-tuple colour dict as a dense table, uint8 [prod,3]
    export_frame(im=, gt_im=, depth=, gt_depth=, im_semantic=, gt_levels=, labels=, gt_labels=, ...)
                                                                      ONE launch: a dict of uint8 [H,W,3] device tensors
    write_png(path, u8)                                               PIL, host

Every picture holds R, G, B in memory; cv2.imwrite takes B, G, R of the same colours, so the PNG written here shows the reference's
picture.  There is no CPU path for export_frame; the tables are built on the host with numpy, once.
"""
import numpy as np
import torch

from diff_gaussian_rasterization import _abi
from .evaluate import _dev, _plane, tree_levels

_lib = _abi.lib

EXPORT_MAX_JOBS = 8            # HSR_EXPORT_MAX_JOBS
EXPORT_MAX_SIDE = 16384        # HSR_RESAMPLE_MAX_SIDE
COLOR, DEPTH, LABELS, LEVELS, LOGITS = 0, 1, 2, 3, 4      # HSR_EXPORT_*
PICTURES = ("im", "gt_im", "depth", "gt_depth", "im_semantic", "gt_levels", "labels", "gt_labels")
_jet_cache = {}


def jet_colormap(device="cuda"):
    """uint8 [256,3], rows R, G, B: the table of the depth pictures.  Exact integer arithmetic: with c = 3, 2, 1 for R, G, B,
        T(i, c) = clamp(765 - |8 * i - 510 * c|, 0, 510),   value = (T + 1) // 2
    which is 255 * clamp(1.5 - |4 * i / 255 - c|, 0, 1) with halves rounded up.  Entry 0 is (0, 0, 128), entry 255 (128, 0, 0), entry
    96 (2, 255, 254).  RESTATED, NOT PINNED BY cv2: cv2 is not available to this project's tests.  cv2.COLORMAP_JET is believed to be
    this curve; every value on a ramp is an exact half before rounding, and which neighbour cv2's table holds depends on its float
    literals, so ramp entries may differ from cv2's by one grey level.  NOT CHECKED.  The table is an argument of export_frame
    (depth_table), so a caller who has cv2's table can pass it."""
    i = np.arange(256, dtype=np.int64)[:, None]
    c = np.array([3, 2, 1], dtype=np.int64)[None, :]
    t = np.clip(765 - np.abs(8 * i - 510 * c), 0, 510)
    return torch.tensor(((t + 1) // 2).astype(np.uint8), device=device)


def label_colormap(n, device="cuda"):
    """uint8 [n,3], rows R, G, B: imgviz.label_colormap restated (the reference's colors_map_all,
    datasets/gradslam_datasets/replica.py:153).  For j in 0..7, bits 0, 1, 2 of the id go to bit 7 - j of r, g, b, then the id shifts
    right by 3: rows 0..3 are (0,0,0), (128,0,0), (0,128,0), (128,128,0), row 8 is (64,0,0).  imgviz is not available to this
    project's tests: NOT CHECKED against it."""
    n = int(n)
    if n < 1:
        raise ValueError("hsr_utils.export: label_colormap takes n >= 1, not %d" % n)
    ids = np.arange(n, dtype=np.int64)
    table = np.zeros((n, 3), dtype=np.int64)
    for j in range(8):
        for ch in range(3):
            table[:, ch] |= ((ids >> ch) & 1) << (7 - j)
        ids = ids >> 3
    return torch.tensor(table.astype(np.uint8), device=device)


def tuple_colour_table(colour_map_level, level_sizes, wildcard, device="cuda"):
    """The dataset's colour_map_np_level ({tuple of per-level labels: (r, g, b)}) as a dense uint8 [prod(sizes), 3] table over the
    mixed-radix index of evaluate.tree_lookup_table (level 0 most significant), sizes = level_sizes[:-1] as there (the dataset's
    num_semantic, whose last entry is the leaf count).  Entries are assigned in dict order and a later one wins, as the reference's
    loop of masked assignments does.  wildcard=True is semantic_label_vis_replica (utils/eval_helpers.py:92-98, :119-133): a -1 in a
    key matches every label of that level (a key of -1 alone matches every tuple).  wildcard=False is semantic_label_vis (:100-117,
    ScanNet): a key holding -1 matches nothing, since no label is -1.  A key with a label outside its level's range matches nothing;
    rows no key names are black.  Keys may be tuples, lists, arrays or tensors.  Built once on the host."""
    sizes, n = tree_levels(level_sizes)
    strides = [int(np.prod(sizes[l + 1:], dtype=np.int64)) for l in range(len(sizes))]
    table = np.zeros((n, 3), dtype=np.uint8)
    for key, value in colour_map_level.items():
        key = [int(k) for k in (key.tolist() if hasattr(key, "tolist") else key)]
        if len(key) != len(sizes):
            raise RuntimeError("hsr_utils.export: colour key %r has %d levels, level_sizes %d" % (key, len(key), len(sizes)))
        rgb = np.asarray(value.tolist() if hasattr(value, "tolist") else value, dtype=np.int64).reshape(-1)
        if rgb.shape != (3,) or rgb.min() < 0 or rgb.max() > 255:
            raise RuntimeError("hsr_utils.export: the colour of key %r must be three values in 0..255 (got %r)" % (key, value))
        idx = np.zeros(1, dtype=np.int64)
        for k, s, stride in zip(key, sizes, strides):
            if k == -1 and wildcard:
                choices = np.arange(s, dtype=np.int64)
            elif 0 <= k < s:
                choices = np.array([k], dtype=np.int64)
            else:
                choices = np.zeros(0, dtype=np.int64)
            idx = (idx[:, None] + choices[None, :] * stride).reshape(-1)
        table[idx] = rgb.astype(np.uint8)
    return torch.tensor(table, device=device)


def _table(t, what, rows=None):
    t = _dev(t, what, torch.uint8)
    if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] < 1 or (rows is not None and t.shape[0] != rows):
        raise RuntimeError("hsr_utils.export: %s must be uint8 [%s,3] (got %s)" % (what, "n" if rows is None else rows, tuple(t.shape)))
    return t


def export_frame(*, im=None, gt_im=None, depth=None, gt_depth=None, im_semantic=None, gt_levels=None, labels=None, gt_labels=None,
                 depth_table=None, depth_range=(0.0, 6.0), level_sizes=None, tuple_table=None, label_table=None):
    """The pictures of one frame from ONE hsr_frame_export launch: a dict, keyed like the arguments given, of uint8 [H,W,3] device
    tensors (R, G, B).  Any subset of
      im, gt_im           float32 [3,H,W]: clamp to 0..1, * 255, round half to even (utils/eval_helpers.py:1520-1527, :1531-1536);
      depth, gt_depth     float32 [1,H,W] or [H,W]: depth_table[int(clip((d - lo) / (hi - lo), 0, 1) * 255)] with (lo, hi) =
                          depth_range (the reference: 0, 6) and depth_table uint8 [256,3] (default jet_colormap) (:1522-1526);
      im_semantic         float32 [K,H,W] rendered semantic map: the level labels of evaluate.semantic_labels(mode="tree"), coloured
                          by tuple_table (tuple_colour_table) with level_sizes as there (:1314-1327);
      gt_levels           int64 [L,H,W] ground-truth level planes (the frame's semantic_label_gt[:-1]): coloured by tuple_table;
                          a label outside its level gives black (:1345-1353);
      labels, gt_labels   int32 or int64 [H,W] or [1,H,W] class maps: label_table[label] (label_colormap), black outside the table
                          (:1054, :1070, :1335).
    Inputs are checked as evaluate's are: float32 / int dtypes as listed, on one HIP device, one H x W.  No host synchronisation, no
    copy of a contiguous input; include/ext/hsr_frame_export.h states every rule step by step.  There is no CPU path."""
    given = [(k, v) for k, v in zip(PICTURES, (im, gt_im, depth, gt_depth, im_semantic, gt_levels, labels, gt_labels)) if v is not None]
    if not given:
        raise RuntimeError("hsr_utils.export: export_frame needs at least one picture")
    first = given[0][1]
    if not isinstance(first, torch.Tensor) or first.dim() < 2:
        raise RuntimeError("hsr_utils.export: %s must be a tensor of at least two dimensions" % given[0][0])
    H, W = int(first.shape[-2]), int(first.shape[-1])
    if not (1 <= H <= EXPORT_MAX_SIDE and 1 <= W <= EXPORT_MAX_SIDE):
        raise ValueError("hsr_utils.export: export_frame sides must be 1..%d; got %dx%d" % (EXPORT_MAX_SIDE, H, W))
    sizes = n_tuples = None
    if im_semantic is not None or gt_levels is not None:
        if level_sizes is None or tuple_table is None:
            raise RuntimeError("hsr_utils.export: im_semantic and gt_levels need level_sizes and tuple_table")
        sizes, n_tuples = tree_levels(level_sizes)
        tuple_table = _table(tuple_table, "tuple_table", n_tuples)
    if labels is not None or gt_labels is not None:
        if label_table is None:
            raise RuntimeError("hsr_utils.export: labels and gt_labels need label_table")
        label_table = _table(label_table, "label_table")
    lo, hi = (float(v) for v in depth_range)
    if depth is not None or gt_depth is not None:
        if not (np.isfinite(np.float32(hi) - np.float32(lo)) and np.float32(hi) - np.float32(lo) > 0):
            raise ValueError("hsr_utils.export: depth_range must be (lo, hi) with a finite hi - lo > 0; got %r" % (depth_range,))
    jobs, keep, out = (_abi.hsr_export_job * len(given))(), [], {}
    dev = None
    for job, (name, t) in zip(jobs, given):
        if name in ("im", "gt_im"):
            t = _dev(t, name)
            if tuple(t.shape) != (3, H, W):
                raise RuntimeError("hsr_utils.export: %s must be [3,%d,%d] (got %s)" % (name, H, W, tuple(t.shape)))
            job.kind = COLOR
        elif name in ("depth", "gt_depth"):
            t = _plane(t, name, H, W)
            if depth_table is None:
                if t.device not in _jet_cache:
                    _jet_cache[t.device] = jet_colormap(t.device)
                depth_table = _jet_cache[t.device]
            depth_table = _table(depth_table, "depth_table", 256)
            job.kind, job.table, job.n, job.lo, job.hi = DEPTH, depth_table.data_ptr(), 256, lo, hi
            keep.append(depth_table)
        elif name == "im_semantic":
            t = _dev(t, name)
            if t.dim() == 4 and t.shape[0] == 1:
                t = t[0]
            if t.dim() != 3 or tuple(t.shape[1:]) != (H, W) or t.shape[0] < sum(sizes):
                raise RuntimeError("hsr_utils.export: im_semantic must be [K,%d,%d] with K >= %d, the levels %s (got %s)"
                                   % (H, W, sum(sizes), sizes, tuple(t.shape)))
            job.kind, job.table, job.n, job.K, job.L = LOGITS, tuple_table.data_ptr(), n_tuples, int(t.shape[0]), len(sizes)
            job.sizes[:len(sizes)] = sizes
        elif name == "gt_levels":
            t = _dev(t, name, torch.int64)
            if tuple(t.shape) != (len(sizes), H, W):
                raise RuntimeError("hsr_utils.export: gt_levels must be [%d,%d,%d] (got %s)" % (len(sizes), H, W, tuple(t.shape)))
            job.kind, job.table, job.n, job.L = LEVELS, tuple_table.data_ptr(), n_tuples, len(sizes)
            job.sizes[:len(sizes)] = sizes
        else:      # labels, gt_labels: an int64 map is one level of label_table's size — the same rule, without a conversion
            wide = isinstance(t, torch.Tensor) and t.dtype == torch.int64
            t = _plane(t, name, H, W, torch.int64 if wide else torch.int32)
            job.kind, job.table, job.n = (LEVELS if wide else LABELS), label_table.data_ptr(), int(label_table.shape[0])
            if wide:
                job.L, job.sizes[0] = 1, int(label_table.shape[0])
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError("hsr_utils.export: %s is on %s, the first picture on %s" % (name, t.device, dev))
        o = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        job.src, job.out = t.data_ptr(), o.data_ptr()
        keep.append(t)
        out[name] = o
    for tab, what in ((tuple_table, "tuple_table"), (label_table, "label_table"), (depth_table, "depth_table")):
        if tab is not None and tab.device != dev:
            raise RuntimeError("hsr_utils.export: %s is on %s, the pictures on %s" % (what, tab.device, dev))
    _abi.call(_lib.hsr_frame_export, "hsr_frame_export", dev, H, W, len(given), jobs)
    return out


def write_png(path, u8):
    """one picture (uint8 [H,W,3], R G B; a tensor anywhere or a numpy array) as a PNG file: PIL on the host, one device-to-host copy"""
    from PIL import Image
    a = u8.detach().cpu().numpy() if isinstance(u8, torch.Tensor) else np.asarray(u8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise RuntimeError("hsr_utils.export: write_png takes uint8 [H,W,3] (got %s %s)" % (a.dtype, a.shape))
    Image.fromarray(np.ascontiguousarray(a)).save(path, format="PNG")


__all__ = ["jet_colormap", "label_colormap", "tuple_colour_table", "export_frame", "write_png", "PICTURES"]
