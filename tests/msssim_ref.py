"""Checker of the multi-scale SSIM (include/ext/hsr_msssim.h): two restatements of the header's steps that share no code, and the
frames the MS-SSIM suites score.

    msssim_torch(x, y, dtype, pool_padding=True)   torch conv2d / avg_pool2d
    msssim_scipy(x, y)                             scipy.ndimage / scipy.signal, float64

Both take the two images [3,H,W] ALREADY multiplied by the masks (values in [0, 1]) and return (score, table): table[s, c] =
(mean cs, mean ssim) of scale s and channel c before the relu, float64 [5,3,2].  They restate the definition (Wang, Simoncelli,
Bovik 2003) with the arguments of the reference's call (data_range 1, size_average); the reference's package is not importable
here, so nothing below is pinned by it.  pool_padding=False is the negative control: a pool that drops the odd row / column
instead of padding in front of it.
"""
import numpy as np
import scipy.ndimage
import scipy.signal
import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
C1, C2 = 0.01 ** 2, 0.03 ** 2

# (H, W): the smallest legal size (a 1x1 last map); odd and even mixed; a second odd / even mix; the flagship frame
SMALL_SIZES = ((161, 161), (161, 178), (176, 193))
LARGE_SIZE = (680, 1200)
KINDS = ("noise", "texture", "masked")


def msssim_torch(x, y, dtype, pool_padding=True):
    x, y = x.to(dtype)[None], y.to(dtype)[None]
    i = torch.arange(11, dtype=dtype, device=x.device) - 5
    g = torch.exp(-(i * i) / (2 * 1.5 ** 2))
    g = g / g.sum()
    w_row, w_col = g.view(1, 1, 1, 11).repeat(3, 1, 1, 1), g.view(1, 1, 11, 1).repeat(3, 1, 1, 1)

    def blur(t):
        return F.conv2d(F.conv2d(t, w_row, groups=3), w_col, groups=3)

    table = torch.full((5, 3, 2), float("nan"), dtype=torch.float64, device=x.device)
    for s in range(5):
        if min(x.shape[2:]) < 11:      # only the negative control gets here
            break
        m1, m2 = blur(x), blur(y)
        s1, s2, s12 = blur(x * x) - m1 * m1, blur(y * y) - m2 * m2, blur(x * y) - m1 * m2
        cs = (2 * s12 + C2) / (s1 + s2 + C2)
        ss = (2 * m1 * m2 + C1) / (m1 * m1 + m2 * m2 + C1) * cs
        table[s, :, 0], table[s, :, 1] = cs.mean((0, 2, 3)).double(), ss.mean((0, 2, 3)).double()
        if s < 4:
            pad = [n % 2 for n in x.shape[2:]] if pool_padding else 0
            x, y = F.avg_pool2d(x, 2, padding=pad), F.avg_pool2d(y, 2, padding=pad)
    v = torch.relu(torch.cat([table[:4, :, 0], table[4:, :, 1]]).to(dtype))
    score = torch.prod(v ** torch.tensor(WEIGHTS, dtype=dtype, device=x.device).view(5, 1), 0).mean()
    return float(score), table.cpu().numpy()


def msssim_scipy(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    k = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-k ** 2 / 4.5)
    g /= g.sum()

    def valid_blur(plane):
        out = scipy.ndimage.correlate1d(plane, g, axis=1, mode="constant")
        out = scipy.ndimage.correlate1d(out, g, axis=0, mode="constant")
        return out[5:-5, 5:-5]

    def halve(plane):
        front = ((plane.shape[0] % 2, 0), (plane.shape[1] % 2, 0))
        sums = scipy.signal.convolve2d(np.pad(plane, front), np.ones((2, 2)), mode="valid")
        return sums[::2, ::2] / 4.0

    table = np.zeros((5, 3, 2))
    for c in range(3):
        a, b = x[c], y[c]
        for s in range(5):
            ma, mb = valid_blur(a), valid_blur(b)
            va, vb, cab = valid_blur(a * a) - ma * ma, valid_blur(b * b) - mb * mb, valid_blur(a * b) - ma * mb
            contrast = (2 * cab + C2) / (va + vb + C2)
            luminance = (2 * ma * mb + C1) / (ma * ma + mb * mb + C1)
            table[s, c] = contrast.mean(), (luminance * contrast).mean()
            if s < 4:
                a, b = halve(a), halve(b)
    per_scale = np.concatenate([table[:4, :, 0], table[4:, :, 1]])
    score = np.prod(np.maximum(per_scale, 0.0) ** np.asarray(WEIGHTS)[:, None], axis=0).mean()
    return float(score), table


def make_frame(H, W, kind, seed):
    """One frame on the CPU, float32: im, gt_im [3,H,W], gt_depth, final_opacity [H,W], sil_thres.
      noise    uniform noise;
      texture  the noise blurred by a 9x9 box, scaled by 3 and wrapped into [0, 1): smooth patches with sharp edges;
      masked   the texture, with a gt_depth that is 0 on the top third and on 30 % of the other pixels.
    gt_im = clamp(im + 0.15 N(0, 1)).  The silhouette (used when a test passes it on) drops the left eighth and ~1 pixel in 6."""
    g = torch.Generator().manual_seed(seed)
    im = torch.rand(3, H, W, generator=g)
    if kind != "noise":
        im = F.avg_pool2d(im[None], 9, 1, 4)[0] * 3 % 1
    gt = (im + 0.15 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    depth = 0.5 + 4 * torch.rand(H, W, generator=g)
    if kind == "masked":
        depth = depth * (torch.rand(H, W, generator=g) > 0.3)
        depth[: H // 3] = 0
    opacity = 0.75 + 0.3 * torch.rand(H, W, generator=g)
    opacity[:, : W // 8] = 0.1
    return im.contiguous(), gt.contiguous(), depth.contiguous(), opacity.contiguous(), 0.8


def masked(im, gt, depth, opacity=None, sil_thres=None):
    """the two images as the reference hands them to its ms_ssim call: times presence (silhouette branch only), times valid"""
    valid = (depth > 0).float()
    if opacity is not None:
        pres = (opacity > sil_thres).float()
        im, gt = im * pres, gt * pres
    return im * valid, gt * valid


def cases():
    """(id, H, W, kind, silhouette): the three small sizes with every kind, silhouette on and off; the flagship frame once"""
    out = []
    for H, W in SMALL_SIZES:
        for kind in KINDS:
            for sil in (False, True):
                out.append(("%dx%d-%s-%s" % (H, W, kind, "sil" if sil else "nosil"), H, W, kind, sil))
    out.append(("%dx%d-masked-sil" % LARGE_SIZE, LARGE_SIZE[0], LARGE_SIZE[1], "masked", True))
    return out


_cache = {}


def reference(case):
    """(im, gt, depth, opacity, sil_thres, score64, table64) of a case, computed once per session; callers must not modify it"""
    if case[0] not in _cache:
        _id, H, W, kind, sil = case
        im, gt, depth, opacity, thres = make_frame(H, W, kind, seed=H * 4096 + W + KINDS.index(kind))
        x, y = masked(im, gt, depth, opacity if sil else None, thres)
        score, table = msssim_torch(x, y, torch.float64)
        _cache[case[0]] = (im, gt, depth, opacity, thres, score, table)
    return _cache[case[0]]
