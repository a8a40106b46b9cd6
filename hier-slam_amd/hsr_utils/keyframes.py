"""Keyframe selection by overlap for the mapping window, with the reference's function name (utils/keyframe_selection.py:40-96, called
at scripts/hierslam.py:1966 for every mapped frame), on the GPU (include/hsr_keyframes.h).

    keyframe_selection_overlap(gt_depth, w2c, intrinsics, keyframe_list, k, pixels=1600)   the reference's arguments and return value
    overlap_counts(gt_depth, w2c, intrinsics, keyframe_list, pixels=1600)                  the numbers behind it, as device tensors
    KeyframePoses                                                                          a growing device table of est_w2c
    mapping_window(selected, keyframe_list, time_idx)                                      scripts/hierslam.py:1967-1974

The random streams are the reference's, drawn in its order: ONE torch.randint(n_valid, (pixels,)) on the CPU default generator (:58),
then ONE np.random.permutation over the ids with a non-zero count (:93).  Under equal seeds the returned list is the reference's.
Five kernel launches per call whatever the number of keyframes; the host reads n_valid (it bounds randint), the counts at the end, and
fx, fy, cx, cy when the intrinsics live on the device.  There is no CPU path.
"""
import numpy as np
import torch

from diff_gaussian_rasterization import _abi

_lib = _abi.lib

MAX_POINTS = 4096
EDGE = 20            # utils/keyframe_selection.py:78


def _depth_plane(gt_depth):
    if not isinstance(gt_depth, torch.Tensor) or not gt_depth.is_cuda or gt_depth.dtype != torch.float32:
        raise RuntimeError("hsr_utils.keyframes: gt_depth must be a float32 tensor on a HIP device; there is no CPU path")
    if gt_depth.dim() != 3 or gt_depth.shape[0] < 1:
        raise RuntimeError("hsr_utils.keyframes: gt_depth must be [1,H,W] (got %s)" % (tuple(gt_depth.shape),))
    return gt_depth[0].contiguous()


class KeyframePoses:
    """The keyframes' est_w2c as one device table [capacity,4,4] (float32) that grows by doubling: append() is one small copy per new
    keyframe, where stacking the list of dicts costs one per keyframe per call."""

    def __init__(self, device="cuda", capacity=64):
        self._table = torch.zeros((max(1, int(capacity)), 4, 4), dtype=torch.float32, device=device)
        self._n = 0

    def __len__(self):
        return self._n

    def append(self, est_w2c):
        if tuple(est_w2c.shape) != (4, 4):
            raise RuntimeError("hsr_utils.keyframes: est_w2c must be [4,4] (got %s)" % (tuple(est_w2c.shape),))
        if self._n == self._table.shape[0]:
            grown = torch.zeros((2 * self._n, 4, 4), dtype=torch.float32, device=self._table.device)
            grown[:self._n] = self._table
            self._table = grown
        self._table[self._n] = est_w2c.detach().to(device=self._table.device, dtype=torch.float32)
        self._n += 1

    def table(self, n=None):
        """the first n poses ([n,4,4], a view; default: all)"""
        n = self._n if n is None else int(n)
        if not 0 <= n <= self._n:
            raise RuntimeError("hsr_utils.keyframes: %d keyframes asked for, the table holds %d" % (n, self._n))
        return self._table[:n]


def _poses(keyframe_list, n_keyframes, dev):
    if isinstance(keyframe_list, KeyframePoses):
        t = keyframe_list.table(n_keyframes)
        if t.device != dev:
            raise RuntimeError("hsr_utils.keyframes: the KeyframePoses table lives on %s, gt_depth on %s" % (t.device, dev))
        return t
    if n_keyframes is not None:
        keyframe_list = keyframe_list[:int(n_keyframes)]
    if len(keyframe_list) == 0:
        return torch.zeros((0, 4, 4), dtype=torch.float32, device=dev)
    return torch.stack([kf['est_w2c'].detach() for kf in keyframe_list]).to(device=dev, dtype=torch.float32).contiguous()   # :67


def round_keys(values):
    """|torch.round(values, decimals=4)| as the removal rule evaluates it (:28), element-wise; float32 on the device."""
    if not values.is_cuda or values.dtype != torch.float32:
        raise RuntimeError("hsr_utils.keyframes: values must be a float32 tensor on a HIP device; there is no CPU path")
    v = values.contiguous()
    out = torch.empty_like(v)
    _abi.call(_lib.hsr_kf_round_keys, "hsr_kf_round_keys", v.device, v.numel(), v.data_ptr(), out.data_ptr())
    return out


def valid_row_prefix(gt_depth):
    """int32 [H+1] on the device: the number of pixels with depth > 0 above each row; [H] = n_valid (:56)."""
    d = _depth_plane(gt_depth)
    H, W = d.shape
    prefix = torch.empty(H + 1, dtype=torch.int32, device=d.device)
    _abi.call(_lib.hsr_kf_valid_rows, "hsr_kf_valid_rows", d.device, H, W, d.data_ptr(), prefix.data_ptr())
    return prefix


def sample_points(gt_depth, w2c, intrinsics, ranks, row_prefix=None):
    """The reference's sampled cloud for the given ranks into the valid pixels (int64, as torch.randint yields them; :59, :10-37).
    Returns (pts [n,3] with the survivors compacted in front, pixels int32 [n,2] (row, col), keep uint8 [n], count int32 [1]), all on the
    device; the host reads nothing but fx, fy, cx, cy (and those only when the intrinsics live on the device)."""
    d = _depth_plane(gt_depth)
    H, W = d.shape
    dev = d.device
    n = int(ranks.numel())
    if not 1 <= n <= MAX_POINTS:
        raise RuntimeError("hsr_utils.keyframes: %d sampled pixels; 1..%d are supported" % (n, MAX_POINTS))
    if row_prefix is None:
        row_prefix = valid_row_prefix(gt_depth)
    r = ranks.to(device=dev, dtype=torch.int64).contiguous()
    K = intrinsics.detach().float().cpu()
    c2w = torch.inverse(w2c.detach().float()).to(dev).contiguous()           # :24
    pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
    pix = torch.empty((n, 2), dtype=torch.int32, device=dev)
    keep = torch.empty((n,), dtype=torch.uint8, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    sc = torch.empty(int(_lib.hsr_kf_sample_scratch_bytes(n)), dtype=torch.uint8, device=dev)
    _abi.call(_lib.hsr_kf_sample_points, "hsr_kf_sample_points", dev, H, W, d.data_ptr(), row_prefix.data_ptr(), n, r.data_ptr(),
              float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), c2w.data_ptr(), pts.data_ptr(), pix.data_ptr(), keep.data_ptr(),
              count.data_ptr(), sc.data_ptr(), sc.numel())
    return pts, pix, keep, count


def project_counts(pts, count, poses, intrinsics, W, H):
    """int32 [n_kf] on the device: per keyframe, how many of the first `count` (device int32 [1], or None for all) rows of pts fall
    inside its image (:69-81)."""
    dev = pts.device
    n_kf = int(poses.shape[0])
    out = torch.empty(n_kf, dtype=torch.int32, device=dev)
    if n_kf == 0:
        return out
    p = poses.to(device=dev, dtype=torch.float32).contiguous()
    K = intrinsics.detach().to(device=dev, dtype=torch.float32).contiguous()
    if K.numel() != 9:
        raise RuntimeError("hsr_utils.keyframes: intrinsics must be [3,3] (got %s)" % (tuple(intrinsics.shape),))
    _abi.call(_lib.hsr_kf_overlap_counts, "hsr_kf_overlap_counts", dev, int(pts.shape[0]), None if count is None else count.data_ptr(),
              pts.data_ptr(), n_kf, p.data_ptr(), K.data_ptr(), int(W), int(H), EDGE, out.data_ptr())
    return out


def _counts(gt_depth, w2c, intrinsics, keyframe_list, pixels, n_keyframes):
    d = _depth_plane(gt_depth)
    H, W = d.shape
    prefix = valid_row_prefix(gt_depth)
    n_valid = int(prefix[H].item())                                          # the host read that torch.randint's bound needs
    indices = torch.randint(n_valid, (pixels,))                              # :58 — the CPU default generator; raises for n_valid == 0
    pts, pix, keep, count = sample_points(gt_depth, w2c, intrinsics, indices, prefix)
    poses = _poses(keyframe_list, n_keyframes, d.device)
    return project_counts(pts, count, poses, intrinsics, W, H), count, pts, pix, keep


def overlap_counts(gt_depth, w2c, intrinsics, keyframe_list, pixels=1600, n_keyframes=None, details=False):
    """(counts int32 [n_kf], n_points int32 [1]) on the device: per keyframe the number of sampled points inside its image, and the
    number of points that survived the removal rule; percent_inside (:83) is their quotient.  Draws the ranks exactly as
    keyframe_selection_overlap does.  details=True adds (pts, pixels, keep) of sample_points."""
    counts, count, pts, pix, keep = _counts(gt_depth, w2c, intrinsics, keyframe_list, pixels, n_keyframes)
    return (counts, count, pts, pix, keep) if details else (counts, count)


def keyframe_selection_overlap(gt_depth, w2c, intrinsics, keyframe_list, k, pixels=1600, n_keyframes=None):
    """The reference's selection (utils/keyframe_selection.py:40-96): up to k ids into keyframe_list, a random subset of the keyframes
    that see at least one of `pixels` points sampled from the current frame's valid depth, as a list of numpy integers.
    keyframe_list: the reference's list of dicts with 'est_w2c' (the loop passes keyframe_list[:-1], :1966), or a KeyframePoses with
    n_keyframes = how many of its poses take part (default: all)."""
    counts, _count, _pts, _pix, _keep = _counts(gt_depth, w2c, intrinsics, keyframe_list, pixels, n_keyframes)
    c = counts.cpu().numpy()
    # sorted(..., reverse=True) is stable (:88-89): by count, descending, ties in list order; then the ids with percent_inside > 0 (:91-92)
    order = np.argsort(-c.astype(np.int64), kind="stable")
    selected = [int(i) for i in order if c[i] > 0]
    return list(np.random.permutation(np.array(selected))[:k])              # :93-94


def mapping_window(selected, keyframe_list, time_idx):
    """scripts/hierslam.py:1967-1974: the time indices of the selected keyframes, with the last keyframe and the current frame appended
    to both lists.  Returns (selected_time_idx, selected_keyframes); -1 in the second names the current frame."""
    selected_time_idx = [keyframe_list[frame_idx]['id'] for frame_idx in selected]
    selected = list(selected)
    if len(keyframe_list) > 0:
        selected_time_idx.append(keyframe_list[-1]['id'])
        selected.append(len(keyframe_list) - 1)
    selected_time_idx.append(time_idx)
    selected.append(-1)
    return selected_time_idx, selected


__all__ = ["keyframe_selection_overlap", "overlap_counts", "KeyframePoses", "mapping_window", "sample_points", "project_counts",
           "valid_row_prefix", "round_keys"]
