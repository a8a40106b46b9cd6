"""Raw sensor frames to the tensors the frame loop takes, on the device (include/ext/hsr_frame_ingest.h): what the
reference's dataset objects do between a decoded image and scripts/hierslam.py's loop, once per size
(datasets/gradslam_datasets/basedataset.py:223-227 and scripts/hierslam.py:1777 for the colour image, basedataset.py:248-256 for the
depth map, replica.py:241-299 and :369 for the labels).

    tree_label_table(label_mapping_tree, num_levels, device)      the class-id -> level-labels table the ingest reads
    ingest_frame(color_u8, depth_raw, sizes, png_depth_scale, labels=None, tree_table=None)
                                                                  ONE launch: every size's colour and depth, level 0's label planes
    ingest_frame_undistort(color_u8, depth_raw, sizes, png_depth_scale, camera, distortion, labels=None, tree_table=None)
                                                                  the same, the colour image undistorted inside that launch
                                                                  (include/sensor/hsr_frame_undistort.h, basedataset.py:306-309)

There is no CPU path for the computation; host inputs are copied to the device once each.  hsr_utils.sequence reads a Replica-layout
directory into the raw arrays ingest_frame takes; SlamSession.ingest (hsr_utils.slam) builds a frame dict for step() from them.
"""
import math

import numpy as np
import torch

from diff_gaussian_rasterization import _abi

_lib = _abi.lib

INGEST_MAX_LEVELS = 3          # HSR_INGEST_MAX_LEVELS
INGEST_MAX_SIDE = 16384        # HSR_RESAMPLE_MAX_SIDE
INGEST_MAX_TREE_LEVELS = 16    # HSR_EVAL_MAX_LEVELS
DEPTH_U16, DEPTH_I32, DEPTH_F32 = 0, 1, 2      # HSR_INGEST_DEPTH_*

_LABEL_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)


def tree_label_table(label_mapping_tree, num_levels, device="cuda"):
    """The dataset's label_mapping_tree ({leaf id (int or str): tuple of per-level labels}, the dict evaluate.tree_lookup_table takes)
    as an int32 [n_ids, num_levels] device tensor, n_ids = the largest id + 1: row id holds the id's level labels.  A row the dict does
    not name holds its own id in every column, which is what the ingest writes for an id beyond the table; of two equal keys (3 and
    "3") the later one wins, as the reference's loop of masked assignments does (replica.py:241-247).  Built once on the host."""
    L = int(num_levels)
    if not 1 <= L <= INGEST_MAX_TREE_LEVELS:
        raise ValueError("hsr_utils.frames: tree_label_table takes 1..%d levels, not %d" % (INGEST_MAX_TREE_LEVELS, L))
    rows = {}
    for key, value in label_mapping_tree.items():
        value = [int(v) for v in value]
        if len(value) != L:
            raise RuntimeError("hsr_utils.frames: tree entry %r has %d levels, num_levels is %d" % (key, len(value), L))
        if int(key) < 0:
            raise RuntimeError("hsr_utils.frames: tree entry %r: class ids are not negative" % (key,))
        rows[int(key)] = value
    if not rows:
        raise RuntimeError("hsr_utils.frames: an empty label_mapping_tree")
    n_ids = max(rows) + 1
    if n_ids > 1 << 24:
        raise RuntimeError("hsr_utils.frames: a %d-row label table is too large" % n_ids)
    table = np.repeat(np.arange(n_ids, dtype=np.int64)[:, None], L, axis=1)
    for key, value in rows.items():
        table[key] = value
    if table.min() < -(1 << 31) or table.max() >= 1 << 31:
        raise RuntimeError("hsr_utils.frames: level labels must fit in int32")
    return torch.tensor(table.astype(np.int32), device=device)


def _as_tensor(x, what):
    if torch.is_tensor(x):
        return x
    if isinstance(x, np.ndarray):
        if x.dtype == np.uint16:      # torch has no arithmetic on uint16: the bits travel as int16 and are read as uint16
            x = x.view(np.int16)
        try:
            return torch.from_numpy(np.ascontiguousarray(x))
        except TypeError:
            raise RuntimeError("hsr_utils.frames: %s has dtype %s, which is not taken" % (what, x.dtype))
    raise RuntimeError("hsr_utils.frames: %s must be a torch tensor or a numpy array, not %s" % (what, type(x).__name__))


def ingest_frame(color_u8, depth_raw, sizes, png_depth_scale, labels=None, tree_table=None, _lens=None):
    """hsr_frame_ingest on one raw sensor frame: returns ([(color_i [3,h,w], depth_i [1,h,w]), ...] for the one to three (h, w) of
    `sizes`, labels_out | None).  color_u8 is uint8 [Hs,Ws,3] as decoders deliver it; depth_raw [Hs,Ws] is uint16 (or int16 bits,
    read as uint16), int32 or float32, in sensor units of 1 / png_depth_scale metres; labels, when given, is a [Hs,Ws] class-id image
    of any integer dtype and labels_out is int64 [L + 1, h0, w0] at the FIRST size: one plane per column of tree_table (int32
    [n_ids, L], tree_label_table; None: flat classes, L = 0), then the id itself.  Colour is float32 in 0..1, bilinear in float64 on
    the 8-bit values; depth float32 metres, nearest (include/ext/hsr_frame_ingest.h states every step).  Inputs may be device tensors,
    host tensors or numpy arrays: each host input is copied to the device once (the device of the first device tensor among the
    inputs, else the current one).  One launch, no host synchronisation; there is no CPU path for the computation.
    (_lens: the nine doubles ingest_frame_undistort has checked; the call then goes to hsr_frame_ingest_undistort.)"""
    color, depth = _as_tensor(color_u8, "color_u8"), _as_tensor(depth_raw, "depth_raw")
    lab = None if labels is None else _as_tensor(labels, "labels")
    if color.dtype != torch.uint8 or color.dim() != 3 or color.shape[2] != 3:
        raise RuntimeError("hsr_utils.frames: color_u8 must be uint8 [Hs,Ws,3]; got %s %s" % (color.dtype, tuple(color.shape)))
    Hs, Ws = int(color.shape[0]), int(color.shape[1])
    uint16 = getattr(torch, "uint16", None)
    if depth.dtype == torch.int16 or (uint16 is not None and depth.dtype == uint16):
        depth_type = DEPTH_U16
    elif depth.dtype == torch.int32:
        depth_type = DEPTH_I32
    elif depth.dtype == torch.float32:
        depth_type = DEPTH_F32
    else:
        raise RuntimeError("hsr_utils.frames: depth_raw must be uint16 (or its bits as int16), int32 or float32; got %s" % depth.dtype)
    if tuple(depth.shape) != (Hs, Ws):
        raise RuntimeError("hsr_utils.frames: depth_raw must be [Hs,Ws] = [%d,%d] as the colour image; got %s" % (Hs, Ws, tuple(depth.shape)))
    if lab is not None and (lab.dtype not in _LABEL_DTYPES or tuple(lab.shape) != (Hs, Ws)):
        raise RuntimeError("hsr_utils.frames: labels must be an integer [Hs,Ws] = [%d,%d] image; got %s %s" % (Hs, Ws, lab.dtype, tuple(lab.shape)))
    if tree_table is not None:
        if lab is None:
            raise RuntimeError("hsr_utils.frames: a tree_table without labels")
        if not (torch.is_tensor(tree_table) and tree_table.dtype == torch.int32 and tree_table.dim() == 2 and tree_table.shape[0] >= 1
                and 1 <= tree_table.shape[1] <= INGEST_MAX_TREE_LEVELS):
            raise RuntimeError("hsr_utils.frames: tree_table must be an int32 [n_ids, 1..%d] tensor (tree_label_table)" % INGEST_MAX_TREE_LEVELS)
    sizes = [(int(h), int(w)) for h, w in sizes]
    if not 1 <= len(sizes) <= INGEST_MAX_LEVELS:
        raise ValueError("hsr_utils.frames: ingest_frame takes one to three sizes, not %d" % len(sizes))
    for side in (Hs, Ws) + tuple(v for hw in sizes for v in hw):
        if not 1 <= side <= INGEST_MAX_SIDE:
            raise ValueError("hsr_utils.frames: ingest_frame sides must be 1..%d; got a frame of %dx%d and sizes %s" % (INGEST_MAX_SIDE, Hs, Ws, sizes))
    scale = float(png_depth_scale)
    if not math.isfinite(scale) or scale == 0.0:
        raise ValueError("hsr_utils.frames: ingest_frame: png_depth_scale must be finite and non-zero, not %r" % (png_depth_scale,))
    given = [t for t in (color, depth, lab, tree_table) if t is not None]
    dev = next((t.device for t in given if t.is_cuda), None)
    if dev is None:
        if not torch.cuda.is_available():
            raise RuntimeError("hsr_utils.frames: ingest_frame needs a HIP device; there is no CPU path")
        dev = torch.device("cuda", torch.cuda.current_device())
    color, depth = color.to(dev).contiguous(), depth.to(dev).contiguous()
    if lab is not None:
        lab = lab.to(dev).to(torch.int32).contiguous()
    L = 0
    if tree_table is not None:
        tree_table = tree_table.to(dev).contiguous()
        L = int(tree_table.shape[1])
    out = [(torch.empty((3, h, w), dtype=torch.float32, device=dev), torch.empty((1, h, w), dtype=torch.float32, device=dev)) for h, w in sizes]
    levels = (_abi.hsr_ingest_level * len(sizes))(*[_abi.hsr_ingest_level(h, w, c.data_ptr(), d.data_ptr()) for (h, w), (c, d) in zip(sizes, out)])
    labels_out = None if lab is None else torch.empty((L + 1,) + sizes[0], dtype=torch.int64, device=dev)
    head = (Hs, Ws, color.data_ptr(), depth.data_ptr(), depth_type, scale, None if lab is None else lab.data_ptr(), L,
            None if tree_table is None else tree_table.data_ptr(), 0 if tree_table is None else int(tree_table.shape[0]))
    tail = (len(sizes), levels, None if labels_out is None else labels_out.data_ptr())
    if _lens is None:
        _abi.call(_lib.hsr_frame_ingest, "hsr_frame_ingest", dev, *head, *tail)
    else:
        _abi.call(_lib.hsr_frame_ingest_undistort, "hsr_frame_ingest_undistort", dev, *head, *_lens, *tail)
    return out, labels_out


def ingest_frame_undistort(color_u8, depth_raw, sizes, png_depth_scale, camera, distortion, labels=None, tree_table=None):
    """hsr_frame_ingest_undistort: ingest_frame with the colour image undistorted inside the same single launch (the reference's
    cv2.undistort(color, K, distortion) on the colour image only, basedataset.py:306-309).  camera = (fx, fy, cx, cy) of the SENSOR
    image, in its pixels; distortion holds 4 or 5 Brown-Conrady coefficients in OpenCV's order (k1, k2, p1, p2[, k3]); with 4, k3 is 0.
    More than 5 is a ValueError: the rational and thin-prism terms are not built.  Everything else — the inputs taken, the checks, the
    depth and label rules, the returned ([(color_i [3,h,w], depth_i [1,h,w]), ...], labels_out | None) — is ingest_frame's.  Colour at
    every size is ingest_frame's bilinear rule on the undistorted sensor image, whose pixels are 1/32-pixel bilinear samples of the
    8-bit image with a border of 0 (include/sensor/hsr_frame_undistort.h states every step, and how a reduced size differs from the
    reference's resize-then-undistort).  One launch, no host synchronisation; there is no CPU path for the computation."""
    try:
        cam = [float(v) for v in camera]
    except TypeError:
        cam = []
    if len(cam) != 4:
        raise ValueError("hsr_utils.frames: ingest_frame_undistort: camera must be (fx, fy, cx, cy) of the sensor image; got %r" % (camera,))
    if torch.is_tensor(distortion):
        distortion = distortion.detach().cpu().reshape(-1).tolist()
    coeff = [float(v) for v in np.asarray(distortion, dtype=np.float64).reshape(-1)]
    if len(coeff) > 5:
        raise ValueError("hsr_utils.frames: ingest_frame_undistort takes 4 or 5 distortion coefficients (k1, k2, p1, p2[, k3]); got %d: "
                         "the rational (k4, k5, k6) and thin-prism (s1..s4) terms are not built" % len(coeff))
    if len(coeff) < 4:
        raise ValueError("hsr_utils.frames: ingest_frame_undistort takes 4 or 5 distortion coefficients (k1, k2, p1, p2[, k3]); got %d" % len(coeff))
    coeff = coeff + [0.0] * (5 - len(coeff))
    if not (math.isfinite(cam[0]) and math.isfinite(cam[1]) and cam[0] != 0.0 and cam[1] != 0.0):
        raise ValueError("hsr_utils.frames: ingest_frame_undistort: fx and fy must be finite and non-zero; got %r, %r" % (cam[0], cam[1]))
    if not all(math.isfinite(v) for v in cam[2:] + coeff):
        raise ValueError("hsr_utils.frames: ingest_frame_undistort: cx, cy and the coefficients must be finite; got %r and %r" % (cam[2:], coeff))
    return ingest_frame(color_u8, depth_raw, sizes, png_depth_scale, labels=labels, tree_table=tree_table, _lens=tuple(cam + coeff))


def _int_keys(mapping, what):
    """{int(key): value} of a dict keyed by ints or their strings; of two equal keys the later one wins; no negative key"""
    out = {}
    for key, value in mapping.items():
        if int(key) < 0:
            raise RuntimeError("hsr_utils.frames: %s entry %r: class ids are not negative" % (what, key))
        out[int(key)] = value
    return out


def composed_label_table(class_mapping, label_mapping_tree, num_levels, device="cuda"):
    """The table ingest_frame_planes(..., leaf_column=True) reads: int32 [n_ids, num_levels + 1], row r holding the level labels of
    label_mapping_tree[leaf] and then leaf itself, with leaf = class_mapping.get(r, r); n_ids is the largest key of either dict + 1.

    This is the composition of the reference's two loops of masked assignments on a ScanNet id image: raw id -> NYU40 id
    (datasets/gradslam_datasets/scannet.py:288-290, class_mapping = sequence.scannet_class_mapping), then NYU40 id -> the tree's
    levels (:302-307 for four levels, :325-330 for five, label_mapping_tree = sequence.scannet_tree_annotation), the NYU40 image
    staying as the last plane (:313, :337).  Both loops take their masks from an UNCHANGED copy of the image (semantic_raw in the
    first, semantic_raw_nyu in the second) and write into another, so neither chains: an id that is both a key and another key's
    value is mapped once.  Each loop is therefore a pure lookup, and so is their composition.  A leaf the tree does not name keeps
    the leaf in every level column (the level copies start as the NYU40 image); an id no row holds keeps its raw value on every
    plane, which is what the ingest writes for an id beyond the table.

    class_mapping None is the identity (the reference's "ab" modes, :285-286).  label_mapping_tree None with num_levels 0 gives the
    one-column flat remap (the 'nyu40' mode).  Keys may be ints or their strings, the later of two equal keys wins, and ids and
    labels must fit in int32, as in tree_label_table.  Built once on the host."""
    L = int(num_levels)
    if not 0 <= L <= INGEST_MAX_TREE_LEVELS:
        raise ValueError("hsr_utils.frames: composed_label_table takes 0..%d levels, not %d" % (INGEST_MAX_TREE_LEVELS, L))
    if (label_mapping_tree is None) != (L == 0):
        raise ValueError("hsr_utils.frames: composed_label_table: a label_mapping_tree goes with num_levels >= 1, None with num_levels 0")
    classes = {k: int(v) for k, v in _int_keys(class_mapping or {}, "class_mapping").items()}
    tree = {}
    for key, value in _int_keys(label_mapping_tree or {}, "tree").items():
        value = [int(v) for v in value]
        if len(value) != L:
            raise RuntimeError("hsr_utils.frames: tree entry %r has %d levels, num_levels is %d" % (key, len(value), L))
        tree[key] = value
    if not classes and not tree:
        raise RuntimeError("hsr_utils.frames: an empty class_mapping and an empty label_mapping_tree")
    n_ids = max(list(classes) + list(tree)) + 1
    if n_ids > 1 << 24:
        raise RuntimeError("hsr_utils.frames: a %d-row label table is too large" % n_ids)
    table = np.empty((n_ids, L + 1), dtype=np.int64)
    for r in range(n_ids):
        leaf = classes.get(r, r)
        table[r, :L] = tree.get(leaf, [leaf] * L)
        table[r, L] = leaf
    if table.min() < -(1 << 31) or table.max() >= 1 << 31:
        raise RuntimeError("hsr_utils.frames: class ids and level labels must fit in int32")
    return torch.tensor(table.astype(np.int32), device=device)


def ingest_frame_planes(color_u8, depth_raw, sizes, png_depth_scale, labels=None, label_table=None, leaf_column=False):
    """hsr_frame_ingest_planes: ingest_frame for a frame whose depth and label images have sizes of their own (a ScanNet frame: colour
    and labels 968x1296, depth 480x640).  Returns what ingest_frame returns, ([(color_i [3,h,w], depth_i [1,h,w]), ...] for the one
    to three (h, w) of `sizes`, labels_out | None), from the same kinds of inputs; depth_raw and labels may each be any 2-D shape.
    label_table is int32 [n_ids, L] (tree_label_table) with leaf_column False: L level planes, then the raw id, as ingest_frame.  With
    leaf_column True it is int32 [n_ids, L + 1] (composed_label_table) and the last plane is the row's last column for an id the
    table holds; L may then be 0 (a flat remap, one plane).  Colour is bilinear from its own size, depth and labels nearest from
    theirs (include/ext/hsr_frame_ingest_planes.h states every step).  One launch, no host synchronisation; no CPU path."""
    color, depth = _as_tensor(color_u8, "color_u8"), _as_tensor(depth_raw, "depth_raw")
    lab = None if labels is None else _as_tensor(labels, "labels")
    leaf = bool(leaf_column)
    if color.dtype != torch.uint8 or color.dim() != 3 or color.shape[2] != 3:
        raise RuntimeError("hsr_utils.frames: color_u8 must be uint8 [Hc,Wc,3]; got %s %s" % (color.dtype, tuple(color.shape)))
    uint16 = getattr(torch, "uint16", None)
    if depth.dtype == torch.int16 or (uint16 is not None and depth.dtype == uint16):
        depth_type = DEPTH_U16
    elif depth.dtype == torch.int32:
        depth_type = DEPTH_I32
    elif depth.dtype == torch.float32:
        depth_type = DEPTH_F32
    else:
        raise RuntimeError("hsr_utils.frames: depth_raw must be uint16 (or its bits as int16), int32 or float32; got %s" % depth.dtype)
    if depth.dim() != 2:
        raise RuntimeError("hsr_utils.frames: depth_raw must be a 2-D [Hd,Wd] image; got %s" % (tuple(depth.shape),))
    if lab is not None and (lab.dtype not in _LABEL_DTYPES or lab.dim() != 2):
        raise RuntimeError("hsr_utils.frames: labels must be an integer 2-D [Hl,Wl] image; got %s %s" % (lab.dtype, tuple(lab.shape)))
    if label_table is None:
        if leaf:
            raise RuntimeError("hsr_utils.frames: leaf_column without a label_table")
    else:
        if lab is None:
            raise RuntimeError("hsr_utils.frames: a label_table without labels")
        if not (torch.is_tensor(label_table) and label_table.dtype == torch.int32 and label_table.dim() == 2 and label_table.shape[0] >= 1):
            raise RuntimeError("hsr_utils.frames: label_table must be an int32 2-D [n_ids, columns] tensor (tree_label_table, composed_label_table)")
        L = int(label_table.shape[1]) - int(leaf)
        if L > INGEST_MAX_TREE_LEVELS or L < (0 if leaf else 1):
            raise RuntimeError("hsr_utils.frames: label_table has %d level columns%s; %d..%d are taken" % (
                L, " before its leaf column" if leaf else "", 0 if leaf else 1, INGEST_MAX_TREE_LEVELS))
    sizes = [(int(h), int(w)) for h, w in sizes]
    if not 1 <= len(sizes) <= INGEST_MAX_LEVELS:
        raise ValueError("hsr_utils.frames: ingest_frame_planes takes one to three sizes, not %d" % len(sizes))
    sources = [tuple(int(v) for v in t.shape[:2]) for t in (color, depth, lab) if t is not None]
    for side in tuple(v for hw in sources + sizes for v in hw):
        if not 1 <= side <= INGEST_MAX_SIDE:
            raise ValueError("hsr_utils.frames: ingest_frame_planes sides must be 1..%d; got images of %s and sizes %s" % (INGEST_MAX_SIDE, sources, sizes))
    scale = float(png_depth_scale)
    if not math.isfinite(scale) or scale == 0.0:
        raise ValueError("hsr_utils.frames: ingest_frame_planes: png_depth_scale must be finite and non-zero, not %r" % (png_depth_scale,))
    given = [t for t in (color, depth, lab, label_table) if t is not None]
    dev = next((t.device for t in given if t.is_cuda), None)
    if dev is None:
        if not torch.cuda.is_available():
            raise RuntimeError("hsr_utils.frames: ingest_frame_planes needs a HIP device; there is no CPU path")
        dev = torch.device("cuda", torch.cuda.current_device())
    color, depth = color.to(dev).contiguous(), depth.to(dev).contiguous()
    Hl = Wl = 0
    if lab is not None:
        lab = lab.to(dev).to(torch.int32).contiguous()
        Hl, Wl = sources[2]
    L = 0
    if label_table is not None:
        label_table = label_table.to(dev).contiguous()
        L = int(label_table.shape[1]) - int(leaf)
    out = [(torch.empty((3, h, w), dtype=torch.float32, device=dev), torch.empty((1, h, w), dtype=torch.float32, device=dev)) for h, w in sizes]
    levels = (_abi.hsr_ingest_level * len(sizes))(*[_abi.hsr_ingest_level(h, w, c.data_ptr(), d.data_ptr()) for (h, w), (c, d) in zip(sizes, out)])
    labels_out = None if lab is None else torch.empty((L + 1,) + sizes[0], dtype=torch.int64, device=dev)
    _abi.call(_lib.hsr_frame_ingest_planes, "hsr_frame_ingest_planes", dev, sources[0][0], sources[0][1], color.data_ptr(),
              sources[1][0], sources[1][1], depth.data_ptr(), depth_type, scale, Hl, Wl, None if lab is None else lab.data_ptr(),
              L, None if label_table is None else label_table.data_ptr(), 0 if label_table is None else int(label_table.shape[0]), int(leaf),
              len(sizes), levels, None if labels_out is None else labels_out.data_ptr())
    return out, labels_out


__all__ = ["tree_label_table", "ingest_frame", "composed_label_table", "ingest_frame_planes", "ingest_frame_undistort"]
