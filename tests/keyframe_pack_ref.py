"""A numpy restatement of hsr_keyframe_pack / hsr_keyframe_unpack (include/ext/hsr_keyframe_pack.h): the codes, the three counters and the
inverse, every operation rounded once in the precision the header names.  Not a test; tests/test_keyframe_pack_cpu.py and
tests/test_gpu_keyframe_pack.py import it."""
import numpy as np

F255 = np.float32(255.0)


def ingest_colour(v):
    """float(double(float(v)) / 255.0): hsr_frame_ingest's colour expression on values already rounded to float32"""
    return (np.asarray(v, np.float32).astype(np.float64) / 255.0).astype(np.float32)


def ingest_depth(q, depth_scale):
    """float(double(q) / depth_scale): hsr_frame_ingest's depth expression"""
    with np.errstate(all="ignore"):
        return (np.asarray(q, np.float64) / np.float64(depth_scale)).astype(np.float32)


def _clamp(t, hi):
    """min(max(t, 0), hi) as the kernel writes it: t > 0 ? (t < hi ? t : hi) : 0, so a NaN gives 0"""
    with np.errstate(invalid="ignore"):
        return np.where(t > 0, np.where(t < hi, t, hi), 0).astype(t.dtype)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pack_colour(c):
    """(uint8 codes, number of values whose code does not reproduce them bit for bit)"""
    c = np.ascontiguousarray(c, np.float32)
    with np.errstate(all="ignore"):
        t = c * F255                                   # one float32 product
    v = np.rint(_clamp(t, F255))                       # to nearest, halves to even
    bad = _bits(ingest_colour(v)) != _bits(c)
    return v.astype(np.uint8), int(bad.sum())


def pack_depth(d, depth_scale):
    d = np.ascontiguousarray(d, np.float32)
    with np.errstate(all="ignore"):
        t = d.astype(np.float64) * np.float64(depth_scale)      # one float64 product
    q = np.rint(_clamp(t, np.float64(65535.0)))
    bad = _bits(ingest_depth(q, depth_scale)) != _bits(d)
    return q.astype(np.uint16), int(bad.sum())


def pack_labels(labels):
    labels = np.ascontiguousarray(labels, np.int64)
    bad = (labels < 0) | (labels > 65535)
    return np.clip(labels, 0, 65535).astype(np.uint16), int(bad.sum())


def pack(color, depth, labels, depth_scale):
    """(colour codes | None, depth codes | None, label codes | None, lossy uint32 [3]) for optional groups"""
    lossy = np.zeros(3, np.uint32)
    out = [None, None, None]
    if color is not None:
        out[0], lossy[0] = pack_colour(color)
    if depth is not None:
        out[1], lossy[1] = pack_depth(depth, depth_scale)
    if labels is not None and len(labels):
        out[2], lossy[2] = pack_labels(labels)
    return out[0], out[1], out[2], lossy


def unpack(color_u8, depth_u16, labels_u16, depth_scale):
    return (None if color_u8 is None else ingest_colour(color_u8.astype(np.float32)),
            None if depth_u16 is None else ingest_depth(depth_u16.astype(np.float64), depth_scale),
            None if labels_u16 is None else labels_u16.astype(np.int64))
