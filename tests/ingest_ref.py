"""A numpy restatement of include/ext/hsr_frame_ingest.h, in the header's order: what hsr_frame_ingest must produce bit for bit.

    taps(n_dst, n_src)                      (i0, i1, f) of every destination index along one axis, f in float64
    color_v(color_u8, (h, w))               float64 [3,h,w]: v = top + fy * (bot - top) on the 8-bit taps, in grey levels 0..255
    color(color_u8, (h, w))                 float32 [3,h,w]: float32(v) / float32(255)
    depth(depth_raw, (h, w), scale)         float32 [h,w]: float32(float64(raw[ys][xs]) / scale), nearest
    labels(ids, (h, w), table | None)       int64 [L+1,h,w]: the table's row of a known id, the id itself otherwise, then the id
    independent_v(color_u8, (h, w))         the two restatements of tests/resample_ref.py applied to float64(u8): (torch, scipy)

numpy evaluates a + f * (b - a) on float64 arrays one operation at a time, each rounded once: no fused multiply-add.  The depth and the
label index is (x * Ws) // Wd.  make_frame draws the raw inputs of the suites."""
import numpy as np
import torch

import resample_ref as R


def taps(n_dst, n_src):
    i = np.arange(n_dst, dtype=np.int64)
    n = np.maximum((2 * i + 1) * n_src - n_dst, 0)
    i0 = n // (2 * n_dst)
    i1 = np.minimum(i0 + 1, n_src - 1)
    f = (n - i0 * 2 * n_dst).astype(np.float64) / np.float64(2 * n_dst)
    return i0, i1, f


def color_v(color_u8, size):
    h, w = size
    Hs, Ws, _three = color_u8.shape
    src = np.ascontiguousarray(color_u8.transpose(2, 0, 1)).astype(np.float64)      # [3,Hs,Ws], exact
    x0, x1, fx = taps(w, Ws)
    y0, y1, fy = taps(h, Hs)
    a, b = src[:, y0][:, :, x0], src[:, y0][:, :, x1]
    c, d = src[:, y1][:, :, x0], src[:, y1][:, :, x1]
    fx, fy = fx[None, None, :], fy[None, :, None]
    top = a + fx * (b - a)
    bot = c + fx * (d - c)
    return top + fy * (bot - top)


def color(color_u8, size):
    return color_v(color_u8, size).astype(np.float32) / np.float32(255)


def nearest_index(size, src):
    (h, w), (Hs, Ws) = size, src
    return (np.arange(h, dtype=np.int64) * Hs) // h, (np.arange(w, dtype=np.int64) * Ws) // w


def depth(depth_raw, size, scale):
    ys, xs = nearest_index(size, depth_raw.shape)
    with np.errstate(all="ignore"):
        return (depth_raw[ys[:, None], xs[None, :]].astype(np.float64) / np.float64(scale)).astype(np.float32)


def labels(ids, size, table=None):
    ys, xs = nearest_index(size, ids.shape)
    raw = ids[ys[:, None], xs[None, :]].astype(np.int64)
    planes = []
    if table is not None:
        table = np.asarray(table, dtype=np.int64)
        known = (raw >= 0) & (raw < table.shape[0])
        row = np.where(known, raw, 0)
        planes = [np.where(known, table[row, l], raw) for l in range(table.shape[1])]
    return np.stack(planes + [raw])


def independent_v(color_u8, size):
    """float64 v by torch's F.interpolate and by scipy's map_coordinates on float64(u8) (tests/resample_ref.py, imported as it is)"""
    c = torch.from_numpy(np.ascontiguousarray(color_u8.transpose(2, 0, 1)).astype(np.float64))
    d = torch.zeros(color_u8.shape[:2])
    return R.resample_torch(c, d, size)[0].numpy(), R.resample_scipy(c, d, size)[0].numpy()


def make_frame(Hs, Ws, seed=0):
    """(colour uint8 [Hs,Ws,3], depth uint16 [Hs,Ws] with a block of zeros, 0 and 65535 present where there is room)"""
    g = np.random.default_rng(seed)
    col = g.integers(0, 256, size=(Hs, Ws, 3), dtype=np.uint8)
    dep = g.integers(300, 60000, size=(Hs, Ws)).astype(np.uint16)
    dep[Hs // 4:Hs // 2, Ws // 4:Ws // 2] = 0
    if Hs * Ws > 1:
        dep[Hs - 1, Ws - 1] = 65535
        dep[0, 0] = 0
    return col, dep
