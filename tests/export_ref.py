"""numpy restatement of include/ext/hsr_frame_export.h, rule by rule (the functions color, depth, labels, levels, logits), a second,
literal restatement of the reference's own lines for the two float kinds (color_literal, depth_literal: np.clip, astype, np.rint as
utils/eval_helpers.py:1520-1537 writes them), the per-key mask loops of semantic_label_vis and semantic_label_vis_replica (:92-133) in
torch on the CPU, and the input lists the export suites lay into images.  Host only; tests/test_frame_export_cpu.py compares the two
restatements, tests/test_gpu_frame_export.py compares the kernel against the first, bit for bit."""
import numpy as np
import torch

F255 = np.float32(255.0)
SIZES = ((1, 1), (1, 3), (3, 5), (37, 53), (5, 205))      # 5x205 = 1025: one past whole 4-pixel groups and whole 256-lane blocks


def colour_values():
    """float32: (k + 0.5) / 255 for k = 0..254 — the fp32 product with 255 is exactly k + 0.5 for all of them (asserted by the CPU
    suite), so each is a real tie — then values outside 0..1, the infinities and a NaN, then 0, 1 and plain fractions"""
    ties = ((np.arange(255, dtype=np.float64) + 0.5) / 255.0).astype(np.float32)
    edge = np.array([-1.0, 2.0, np.inf, -np.inf, np.nan, 0.0, 1.0, -0.0, 1e-40, 0.999999, 0.25, 0.5, 0.75, 1.0000001], dtype=np.float32)
    return np.concatenate([ties, edge])


def depth_values():
    """float32: 0, 6, 7, -1, NaN, +-inf, then 6 * k / 255 for k = 0..255 (the values whose index is on the edge of truncation)"""
    edge = np.array([0.0, 6.0, 7.0, -1.0, np.nan, np.inf, -np.inf, 5.9999995, 1e-40, 3.0], dtype=np.float32)
    steps = (6.0 * np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    return np.concatenate([edge, steps])


def lay(values, shape, shift=0):
    """`values` repeated along the flat index of an array of `shape`, starting at values[shift]: every value appears once the array is
    large enough, and the planes of a multi-plane array start at different values"""
    n = int(np.prod(shape))
    idx = (np.arange(n) + shift) % len(values)
    return np.ascontiguousarray(values[idx].reshape(shape))


# ---- the header's rules --------------------------------------------------------------------------------------------------------------
def _clamp01(x):
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, np.where(x < 1, x, np.float32(1)), np.float32(0)).astype(np.float32)      # a NaN fails x > 0


def color(x):
    """float32 [3,H,W] -> uint8 [H,W,3]: clamp, one fp32 product, to nearest with halves to even"""
    assert x.dtype == np.float32 and x.ndim == 3 and x.shape[0] == 3
    p = _clamp01(x) * F255
    assert p.dtype == np.float32
    return np.rint(p).astype(np.uint8).transpose(1, 2, 0).copy()


def depth(d, table, lo=0.0, hi=6.0):
    """float32 [H,W], uint8 [256,3] -> uint8 [H,W,3]: one fp32 subtraction, one fp32 division by the fp32 difference hi - lo, clamp,
    one fp32 product, truncation"""
    assert d.dtype == np.float32 and d.ndim == 2 and table.shape == (256, 3) and table.dtype == np.uint8
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(invalid="ignore"):
        n = (d - lo) / (hi - lo)
    assert n.dtype == np.float32
    idx = (_clamp01(n) * F255).astype(np.int32)
    return table[idx]


def labels(lab, table):
    """int [H,W], uint8 [n,3] -> uint8 [H,W,3]: table[label] inside the table, black outside (no wrap of negative labels)"""
    ok = (lab >= 0) & (lab < len(table))
    out = np.zeros(lab.shape + (3,), dtype=np.uint8)
    out[ok] = table[lab[ok]]
    return out


def levels(lev, sizes, table):
    """int64 [L,H,W], sizes[L], uint8 [prod,3] -> uint8 [H,W,3]: the mixed-radix index, level 0 most significant; black where any
    label is outside its level"""
    assert lev.dtype == np.int64 and len(lev) == len(sizes) and len(table) == int(np.prod(sizes))
    ok = np.ones(lev.shape[1:], dtype=bool)
    idx = np.zeros(lev.shape[1:], dtype=np.int64)
    for plane, s in zip(lev, sizes):
        ok &= (plane >= 0) & (plane < s)
        idx = np.where(ok, idx * s + np.where(ok, plane, 0), 0)
    return labels(np.where(ok, idx, -1), table)


def level_labels(x, sizes):
    """float32 [K,H,W] -> int64 [L,H,W]: per level the FIRST index of the largest value of its planes.  That is the header's label
    (the lowest i with expf(x_i - m) / s == 1 / s) for finite inputs whose values within a level are either equal or apart by more
    than 1e-6, which is all the suites feed: a smaller value then fails the header's own pre-test x_i - m >= -1e-6."""
    out, begin = [], 0
    for s in sizes:
        out.append(np.argmax(x[begin:begin + s], axis=0))
        begin += s
    return np.stack(out).astype(np.int64)


def logits(x, sizes, table):
    return levels(level_labels(x, sizes), sizes, table)


# ---- the reference's lines, literally ------------------------------------------------------------------------------------------------
def color_literal(x):
    """:1520-1521, :1527: torch.clamp(im, 0, 1) -> numpy -> * 255 -> imwrite's conversion to 8 bits, taken as np.rint and a saturating
    cast (OpenCV's cvRound is round-half-to-even); torch.clamp keeps a NaN, which the header sends to 0"""
    viz = torch.clamp(torch.from_numpy(x), 0, 1).permute(1, 2, 0).numpy()
    scaled = viz * 255
    scaled = np.where(np.isnan(scaled), 0, scaled)
    return np.clip(np.rint(scaled), 0, 255).astype(np.uint8)


def depth_literal(d, table, vmin=0, vmax=6):
    """:1522-1526: np.clip((d - vmin) / (vmax - vmin), 0, 1), (. * 255).astype(np.uint8), the colour map's row; np.clip keeps a NaN,
    whose cast is undefined in numpy and 0 in the header"""
    with np.errstate(invalid="ignore"):
        normalized = np.clip((d - vmin) / (vmax - vmin), 0, 1)
    normalized = np.where(np.isnan(normalized), np.float32(0), normalized)
    assert normalized.dtype == np.float32
    return table[(normalized * 255).astype(np.uint8)]


def vis_scannet(label_map_tree, colour_map_level):
    """semantic_label_vis (:100-117): per key, the pixels whose labels equal the key on every level take the key's colour; later keys
    overwrite earlier ones.  label_map_tree: int64 tensor [L,H,W]; keys: tuples or tensors (two tensors may hold one tuple); returns uint8 numpy [H,W,3]"""
    vis = torch.zeros(label_map_tree.shape[1], label_map_tree.shape[2], 3, dtype=torch.uint8)
    for key, value in colour_map_level.items():
        k = torch.as_tensor(key, dtype=label_map_tree.dtype).unsqueeze(1).unsqueeze(1)
        vis[torch.all(label_map_tree == k, dim=0)] = torch.tensor(value, dtype=torch.uint8)
    return vis.numpy()


def vis_replica(label_map_tree, colour_map_level):
    """semantic_label_vis_replica with find_positions (:92-98, :119-133): as above, but the levels where the key holds -1 are left out
    of the comparison"""
    vis = torch.zeros(label_map_tree.shape[1], label_map_tree.shape[2], 3, dtype=torch.uint8)
    planes = label_map_tree.permute(1, 2, 0)
    for key, value in colour_map_level.items():
        k = torch.as_tensor(key, dtype=label_map_tree.dtype)
        named = k != -1
        vis[(planes[:, :, named] == k[named]).all(dim=-1)] = torch.tensor(value, dtype=torch.uint8)
    return vis.numpy()
