"""Two float64 restatements of the frame resample of include/ext/hsr_frame_resample.h that share no code: colour bilinear with half-pixel
centres and a replicated border (cv2.resize INTER_LINEAR, basedataset.py:223-227), depth nearest (INTER_NEAREST, :248-252).

    resample_torch(color, depth, (h, w))   torch F.interpolate: 'bilinear' with align_corners=False, and 'nearest'
    resample_scipy(color, depth, (h, w))   scipy.ndimage.map_coordinates(order=1, mode='nearest') at the explicit half-pixel source
                                           coordinates (x + 0.5) * W / Wd - 0.5, and integer indexing (x * W) // Wd for the depth

Both take CPU tensors color [3,H,W], depth [H,W] or [1,H,W] and return (color float64 [3,h,w], depth [h,w] with the input's dtype and
bits).  tests/test_slam_multires_cpu.py asserts that they agree; tests/test_gpu_frame_resample.py compares the kernel with them."""
import numpy as np
import torch
import torch.nn.functional as F

# H, W -> Hd, Wd: the cases of tests/test_gpu_frame_resample.py
SIZE_PAIRS = (((1, 1), (1, 1)), ((2, 3), (1, 1)), ((5, 7), (5, 7)), ((16, 16), (8, 8)), ((37, 23), (18, 11)), ((37, 23), (19, 12)),
              ((33, 65), (17, 33)), ((48, 64), (97, 130)), ((97, 130), (48, 64)))


def make_frame(H, W, seed=0):
    """colour uniform in [0, 1); depth in [0.5, 5.5) with a block of zeros, one NaN and one inf (where the frame has room for them)"""
    g = torch.Generator().manual_seed(seed)
    color = torch.rand(3, H, W, generator=g)
    depth = torch.rand(H, W, generator=g) * 5 + 0.5
    depth[H // 4:H // 2, W // 4:W // 2] = 0.0
    if H * W > 1:
        depth[H - 1, W - 1] = float("nan")
        depth[0, W // 2] = float("inf")
    return color, depth


def resample_torch(color, depth, size):
    h, w = size
    c = F.interpolate(color.double()[None], size=(h, w), mode="bilinear", align_corners=False, antialias=False)[0]
    H, W = depth.shape[-2:]
    # 'nearest' on the bits: the depth travels as integers so that NaN payloads and inf are copied, not computed with
    bits = depth.reshape(1, 1, H, W).contiguous().view(torch.int32).double()      # |int32| < 2^31: exact in float64
    d = F.interpolate(bits, size=(h, w), mode="nearest")[0, 0].to(torch.int32).view(depth.dtype)
    return c, d


def resample_scipy(color, depth, size):
    from scipy import ndimage
    h, w = size
    H, W = depth.shape[-2:]
    ys = (np.arange(h, dtype=np.float64) + 0.5) * H / h - 0.5
    xs = (np.arange(w, dtype=np.float64) + 0.5) * W / w - 0.5
    coords = np.stack(np.meshgrid(ys, xs, indexing="ij"))
    src = color.double().numpy()
    c = np.stack([ndimage.map_coordinates(src[ch], coords, order=1, mode="nearest") for ch in range(3)])
    yi, xi = (np.arange(h) * H) // h, (np.arange(w) * W) // w
    d = depth.reshape(H, W).numpy()[yi[:, None], xi[None, :]]
    return torch.from_numpy(c), torch.from_numpy(np.ascontiguousarray(d))
