"""A numpy restatement of include/sensor/hsr_frame_undistort.h, in the header's order: what hsr_frame_ingest_undistort must produce bit
for bit, and a second restatement of the undistorted image that shares no expression with the first.

    source(Hs, Ws, camera, dist)                   (us, vs) float64 [Hs,Ws]: the header's association, one rounding per operation
    steps(c)                                       (s, a, nan): i = rint(clip(32 c, -2^30, 2^30)), s = i >> 5, a = i & 31; nan where 32 c is
    undistorted(color_u8, camera, dist)            U float64 [3,Hs,Ws]: the exact 1/32-pixel blend of four 8-bit taps, 0 outside, 0 for a NaN
    color_v(color_u8, (h, w), camera, dist)        float64 [3,h,w]: ingest_ref's lerps on the taps of U (ingest_ref.taps), in grey levels
    color(color_u8, (h, w), camera, dist)          float32 [3,h,w]: float32(v) / float32(255)
    independent_source(Hs, Ws, camera, dist)       (us, vs) in another association: torch float64, u / fx - cx / fx, powers of r2
    independent_undistorted(color_u8, camera, dist)  U by scipy.ndimage.map_coordinates(order=1, mode="grid-constant", cval=0) at the
                                                   coordinates torch rounds to 1/32 pixel

`dist` is (k1, k2, p1, p2, k3), OpenCV's order; `camera` (fx, fy, cx, cy) of the sensor image.  numpy evaluates every operation on
float64 arrays once, rounded once: no fused multiply-add.  Depth and labels are ingest_ref's, unchanged.  CASES are the cases of the
CPU and the GPU suite."""
import numpy as np
import torch

import ingest_ref as I

FR1 = ((517.3, 516.5, 318.6, 255.3), (0.2624, -0.9531, -0.0054, 0.0026, 1.1633))
FR2 = ((520.9, 521.0, 325.1, 249.7), (0.2312, -0.7849, -0.0033, -0.0001, 0.9172))
SMALL_CAMERA = (30.0, 29.0, 18.2, 11.4)
# name -> ((Hs, Ws), camera, dist)
CASES = {
    "480x640-fr1": ((480, 640), FR1[0], FR1[1]),
    "480x640-fr2": ((480, 640), FR2[0], FR2[1]),
    "23x37-fr1": ((23, 37), SMALL_CAMERA, FR1[1]),
    "23x37-outside": ((23, 37), SMALL_CAMERA, (0.9, 0.3, 0.01, -0.02, 0.0)),
    "23x37-inside": ((23, 37), SMALL_CAMERA, (-0.35, 0.12, 0.004, -0.003, -0.02)),
    "5x64": ((5, 64), (50.0, 50.0, 31.5, 2.0), (0.4, 0.0, 0.0, 0.0, 0.0)),
    "1x1": ((1, 1), (1.0, 1.0, 0.3, 0.2), (0.5, 0.0, 0.0, 0.0, 0.0)),
}
SMALL_CASES = ("23x37-fr1", "23x37-outside", "23x37-inside", "5x64", "1x1")
# 9x13 with integer cx, cy: the polynomial overflows everywhere but at the principal point (6, 4), where every coordinate is exact
OVERFLOW = ((1e-3, 1e-3, 6.0, 4.0), (1e300,) * 5)
LIMIT = 2.0 ** 30


def source(Hs, Ws, camera, dist):
    fx, fy, cx, cy = (np.float64(v) for v in camera)
    k1, k2, p1, p2, k3 = (np.float64(v) for v in dist)
    u = np.arange(Ws, dtype=np.float64)[None, :]
    v = np.arange(Hs, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        x = np.broadcast_to((u - cx) / fx, (Hs, Ws))
        y = np.broadcast_to((v - cy) / fy, (Hs, Ws))
        x2, y2 = x * x, y * y
        r2 = x2 + y2
        xy2 = 2.0 * (x * y)
        kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = x * kr + p1 * xy2 + p2 * (r2 + 2.0 * x2)
        yd = y * kr + p1 * (r2 + 2.0 * y2) + p2 * xy2
        return fx * xd + cx, fy * yd + cy


def steps(c):
    with np.errstate(all="ignore"):
        q = c * 32.0
    nan = np.isnan(q)
    i = np.rint(np.clip(np.where(nan, 0.0, q), -LIMIT, LIMIT)).astype(np.int64)      # rint: half to even
    return i >> 5, i & 31, nan


def _tap(src, sy, sx):
    """src [3,Hs,Ws] int64 at (sy, sx), 0 outside"""
    Hs, Ws = src.shape[1:]
    inside = (sy >= 0) & (sy < Hs) & (sx >= 0) & (sx < Ws)
    return np.where(inside[None], src[:, np.clip(sy, 0, Hs - 1), np.clip(sx, 0, Ws - 1)], 0)


def undistorted(color_u8, camera, dist):
    Hs, Ws, _three = color_u8.shape
    src = np.ascontiguousarray(color_u8.transpose(2, 0, 1)).astype(np.int64)
    us, vs = source(Hs, Ws, camera, dist)
    sx, ax, nanx = steps(us)
    sy, ay, nany = steps(vs)
    a, b, c, d = _tap(src, sy, sx), _tap(src, sy, sx + 1), _tap(src, sy + 1, sx), _tap(src, sy + 1, sx + 1)
    n = a * (32 - ax) * (32 - ay) + b * ax * (32 - ay) + c * (32 - ax) * ay + d * ax * ay      # an integer below 2^18
    n = np.where((nanx | nany)[None], 0, n)
    return n.astype(np.float64) / 1024.0


def color_v(color_u8, size, camera, dist):
    h, w = size
    U = undistorted(color_u8, camera, dist)
    _three, Hs, Ws = U.shape
    x0, x1, fx = I.taps(w, Ws)
    y0, y1, fy = I.taps(h, Hs)
    a, b = U[:, y0][:, :, x0], U[:, y0][:, :, x1]
    c, d = U[:, y1][:, :, x0], U[:, y1][:, :, x1]
    fx, fy = fx[None, None, :], fy[None, :, None]
    top = a + fx * (b - a)
    bot = c + fx * (d - c)
    return top + fy * (bot - top)


def color(color_u8, size, camera, dist):
    return color_v(color_u8, size, camera, dist).astype(np.float32) / np.float32(255)


def independent_source(Hs, Ws, camera, dist):
    fx, fy, cx, cy = camera
    k1, k2, p1, p2, k3 = dist
    v, u = torch.meshgrid(torch.arange(Hs, dtype=torch.float64), torch.arange(Ws, dtype=torch.float64), indexing="ij")
    x, y = u / fx - cx / fx, v / fy - cy / fy
    r2 = x ** 2 + y ** 2
    kr = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x ** 2)
    yd = y * kr + p1 * (r2 + 2 * y ** 2) + 2 * p2 * x * y
    return (xd * fx + cx).numpy(), (yd * fy + cy).numpy()


def independent_steps(c):
    """the 1/32-pixel index by torch (torch.round rounds half to even); NaN stays out: (index int64, nan)"""
    q = torch.from_numpy(np.ascontiguousarray(c)) * 32
    nan = torch.isnan(q)
    return torch.round(torch.where(nan, torch.zeros_like(q), q).clamp(-LIMIT, LIMIT)).to(torch.int64).numpy(), nan.numpy()


def independent_undistorted(color_u8, camera, dist):
    from scipy import ndimage
    Hs, Ws, _three = color_u8.shape
    us, vs = independent_source(Hs, Ws, camera, dist)
    (iu, nanx), (iv, nany) = independent_steps(us), independent_steps(vs)
    coords = np.stack([iv.astype(np.float64) / 32.0, iu.astype(np.float64) / 32.0])      # exact
    src = color_u8.astype(np.float64)
    U = np.stack([ndimage.map_coordinates(src[..., ch], coords, order=1, mode="grid-constant", cval=0.0) for ch in range(3)])
    return np.where((nanx | nany)[None], 0.0, U)


def near_half(c, eps=1e-9):
    """where 32 c lies within eps of a half-integer: the only pixels two associations of the coordinates may quantise differently"""
    with np.errstate(all="ignore"):
        q = c * 32.0
        return np.abs(q - np.floor(q) - 0.5) <= eps
