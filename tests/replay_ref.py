"""Restatements for the replay suites, written from the reference's lines (viz_scripts/online_recon_sem_replica.py) and from nothing
under test: the plan as a list of counts, the selection as the boolean index of get_rendervars (:100-158), rgbd2pcd (:220-259) in numpy
float32 with one operation per line, and the 15-byte PLY records through a structured dtype."""
import numpy as np

RECORD = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
assert RECORD.itemsize == 15


def plan_counts(timestep, T):
    """[(ts <= t).sum() for t in range(T)] in float32 (:102: params['timestep'] <= curr_timestep); NaN <= t is False"""
    ts = np.asarray(timestep, np.float32)
    with np.errstate(invalid="ignore"):
        return np.array([int((ts <= np.float32(t)).sum()) for t in range(T)], np.int64)


def select_mask(timestep, step):
    """:102, the boolean index every per-Gaussian tensor is taken with (:109)"""
    with np.errstate(invalid="ignore"):
        return np.asarray(timestep, np.float32) <= np.float32(step)


def rgbd2pcd(depth, k, c2w):
    """:220-239 in float32, every line one correctly rounded operation, in the order (x - CX) / FX, xx * z, then c2w @ [., 1] row by row as
    ((m0 * p0 + m1 * p1) + m2 * p2) + m3 * 1.  depth [H,W]; returns [H*W,3] float32."""
    f = np.float32
    H, W = depth.shape
    fx, fy, cx, cy = f(k[0][0]), f(k[1][1]), f(k[0][2]), f(k[1][2])
    m = np.asarray(c2w, f)
    with np.errstate(all="ignore"):
        xx = np.tile(np.arange(W), H).astype(f)
        yy = np.repeat(np.arange(H), W).astype(f)
        xx = xx - cx
        xx = xx / fx
        yy = yy - cy
        yy = yy / fy
        z = np.ascontiguousarray(depth, f).reshape(-1)
        p0 = xx * z
        p1 = yy * z
        p2 = z
        out = np.empty((H * W, 3), f)
        for r in range(3):
            a = m[r, 0] * p0
            b = m[r, 1] * p1
            s = a + b
            c = m[r, 2] * p2
            s = s + c
            d = m[r, 3] * f(1.0)
            out[:, r] = s + d
    return out


def records(points, picture):
    """the body of the PLY file: x y z as little-endian float32, red green blue from picture [H,W,3] uint8; returns uint8 [n*15]"""
    rec = np.empty(points.shape[0], RECORD)
    rec["x"], rec["y"], rec["z"] = points[:, 0], points[:, 1], points[:, 2]
    rgb = np.asarray(picture, np.uint8).reshape(-1, 3)
    rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    return np.frombuffer(rec.tobytes(), np.uint8)


def same_floats(a, b):
    """bit-equal, NaNs compared as 'is NaN' (a NaN's payload and sign are not part of the contract)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def camera_centres(w2cs):
    """:348"""
    return np.stack([np.linalg.inv(m)[:3, 3] for m in w2cs])


def trajectory_lines(n):
    """make_lineset (:167-169) with num_lines = 1"""
    pt_indices = np.arange(n)
    return np.ascontiguousarray(np.stack((pt_indices, pt_indices - 1), -1)[1:], np.int32)
