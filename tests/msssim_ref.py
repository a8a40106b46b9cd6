"""Checker of the multi-scale SSIM (include/ext/hsr_msssim.h): two restatements of the header's steps that share no code, and the
frames the MS-SSIM suites score.

    msssim_torch(x, y, dtype, pool_padding=True)   torch conv2d / avg_pool2d
    msssim_scipy(x, y)                             scipy.ndimage / scipy.signal, float64

and, for the suites that look below the whole-map means (the pyramid bit for bit, the sums of each 32x32 tile of the maps):

    scratch_layout(H, W)                           the header's scratch layout, restated
    pyramid_fp32(x, y)                             levels 1 to 4 in float32 with the header's pool arithmetic, explicit slices
    levels / level_maps / scale_maps(x, y, dtype)  the per-pixel cs and ssim maps of the 5 scales
    tile_sums(map)                                 float64 sums over the header's tiles
    tile_reference(case)                           all of it for one case, computed once per session

Both take the two images [3,H,W] ALREADY multiplied by the masks (values in [0, 1]) and return (score, table): table[s, c] =
(mean cs, mean ssim) of scale s and channel c before the relu, float64 [5,3,2].  They restate the definition (Wang, Simoncelli,
Bovik 2003) with the arguments of the reference's call (data_range 1, size_average); the reference's package is not importable
here, so nothing below is pinned by it.  pool_padding=False is the negative control: a pool that drops the odd row / column
instead of padding in front of it.
"""
import math

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
# kinds only the tile suite scores: the seed of a frame is H * 4096 + W + ALL_KINDS.index(kind)
ALL_KINDS = KINDS + ("anti", "anti1")
TILE = 32
# the tile suite's sizes: on each axis, at level 0 and again at a level 1 to 3, a size with (n - 10) % 32 == 0 (the last tile owns
# 42 rows / columns), an odd one with == 1 (a last tile of one output), an odd one with == 31, another even and another odd one, and
# a level of exactly 42 (a single tile that owns all of it): tests/test_msssim_cpu.py test_tile_sizes_cover_every_class
#   161 -> 81 41 21 11    170 -> 85 43 22 11    171 -> 86 43 22 11    201 -> 101 51 26 13    330 -> 165 83 42 21
TILE_SIZES = ((161, 170), (170, 161), (171, 201), (201, 330), (330, 171), (161, 1200))


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
      masked   the texture, with a gt_depth that is 0 on the top third and on 30 % of the other pixels;
      anti     the noise with gt_im = 1 - im: every mean cs of scales 0 to 3 is negative, the relu sets the score to exactly 0;
      anti1    the noise with only channel 1 of gt_im replaced by 1 - im[1]: that channel contributes 0, the others do not.
    gt_im = clamp(im + 0.15 N(0, 1)) otherwise.  The silhouette (used when a test passes it on) drops the left eighth and ~1 pixel in 6."""
    g = torch.Generator().manual_seed(seed)
    im = torch.rand(3, H, W, generator=g)
    if kind in ("texture", "masked"):
        im = F.avg_pool2d(im[None], 9, 1, 4)[0] * 3 % 1
    gt = (im + 0.15 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    if kind == "anti":
        gt = 1 - im
    elif kind == "anti1":
        gt[1] = 1 - im[1]
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
        im, gt, depth, opacity, thres = make_frame(H, W, kind, seed=H * 4096 + W + ALL_KINDS.index(kind))
        x, y = masked(im, gt, depth, opacity if sil else None, thres)
        score, table = msssim_torch(x, y, torch.float64)
        _cache[case[0]] = (im, gt, depth, opacity, thres, score, table)
    return _cache[case[0]]


# ---------------------------------------------------------------- below the means: scratch layout, pyramid, maps, tile sums
def level_sizes(H, W):
    sizes = [(H, W)]
    for _ in range(4):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    return sizes


def scratch_layout(H, W):
    """the scratch layout as include/ext/hsr_msssim.h states it (restated by hand, the C code is not read):
      sizes[s]      (h, w) of level s
      pyr[s]        float offset of level s = 1..4 from byte 0: x planes [3][h][w], then y planes
      part_base     byte offset of the partials: the next 256-byte boundary after the pyramid
      tiles[s]      (tiles_y, tiles_x) of scale s
      part[s]       double offset of scale s from part_base: [tile_y * tiles_x + tile_x][channel][cs, ssim]
      bytes         the whole size, the partials rounded up to 256 bytes too"""
    sizes = level_sizes(H, W)
    pyr, floats = {}, 0
    for s in range(1, 5):
        pyr[s] = floats
        floats += 6 * sizes[s][0] * sizes[s][1]
    tiles = [(-(-(h - 10) // TILE), -(-(w - 10) // TILE)) for h, w in sizes]
    part, doubles = [], 0
    for ty, tx in tiles:
        part.append(doubles)
        doubles += 6 * ty * tx
    part_base = -(-4 * floats // 256) * 256
    return dict(sizes=sizes, pyr=pyr, pyr_floats=floats, part_base=part_base, tiles=tiles, part=part, part_doubles=doubles,
                bytes=part_base + -(-8 * doubles // 256) * 256)


def pool(t, padding=True):
    """the header's 2x2 pool of [..., h, w] in t's dtype: zero padding of (size % 2) in front of each axis, (((a00 + a01) + a10) + a11)
    * 0.25 with one rounding per operation.  padding=False is the negative control that drops the odd row / column instead."""
    h, w = t.shape[-2:]
    t = F.pad(t, (w % 2, 0, h % 2, 0)) if padding else t[..., : h - h % 2, : w - w % 2]
    return (((t[..., 0::2, 0::2] + t[..., 0::2, 1::2]) + t[..., 1::2, 0::2]) + t[..., 1::2, 1::2]) * 0.25


def levels(x, y, dtype, pool_padding=True):
    """[(x_s, y_s)] for s = 0..4 in dtype, from the two masked images [3,H,W]"""
    out = [(x.to(dtype), y.to(dtype))]
    for _ in range(4):
        out.append((pool(out[-1][0], pool_padding), pool(out[-1][1], pool_padding)))
    return out


def pyramid_fp32(x, y, pool_padding=True):
    """levels 1 to 4 of the two masked float32 images as the kernel must write them, bit for bit: [(x_s, y_s)], s = 1..4"""
    assert x.dtype == y.dtype == torch.float32
    return levels(x, y, torch.float32, pool_padding)[1:]


def window(dtype):
    """the 11 taps as Python floats: exp(-(i - 5)^2 / (2 * 1.5^2)) rounded to dtype, summed in dtype in index order, each divided by the sum"""
    one = torch.ones((), dtype=dtype)
    g = [one * math.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(11)]
    total = g[0]
    for v in g[1:]:
        total = total + v
    return [float(v / total) for v in g]


def blur(t, g):
    """the valid separable filter of [..., h, w] with explicit slices, in t's dtype: along the rows, then along the columns, the taps
    in index order, one rounding per product and per sum.  Only elementwise IEEE operations: the same bits on every host, which a
    library convolution (whose summation order depends on the CPU) does not promise"""
    for axis in (-1, -2):
        n = t.shape[axis] - 10
        acc = t.narrow(axis, 0, n) * g[0]
        for k in range(1, 11):
            acc = acc + t.narrow(axis, k, n) * g[k]
        t = acc
    return t


def level_maps(xs, ys):
    """(cs, ssim), each [3, h-10, w-10] in the images' dtype: the two per-pixel maps of one level, every step of the header as
    written and rounded once in that dtype (in float32: C1 and C2 rounded to float32 first)"""
    g = window(xs.dtype)
    c1, c2 = float(torch.tensor(C1, dtype=xs.dtype)), float(torch.tensor(C2, dtype=xs.dtype))
    m1, m2 = blur(xs, g), blur(ys, g)
    mu1_sq, mu2_sq, mu12 = m1 * m1, m2 * m2, m1 * m2
    s1, s2, s12 = blur(xs * xs, g) - mu1_sq, blur(ys * ys, g) - mu2_sq, blur(xs * ys, g) - mu12
    cs = (2 * s12 + c2) / (s1 + s2 + c2)
    return cs, (2 * mu12 + c1) / (mu1_sq + mu2_sq + c1) * cs


def scale_maps(x, y, dtype, pool_padding=True):
    """[(cs, ssim)] of the 5 scales, computed in dtype throughout (pyramid included)"""
    return [level_maps(xs, ys) for xs, ys in levels(x, y, dtype, pool_padding)]


def tile_sums(m):
    """float64 [..., tiles_y, tiles_x]: the sums of a map [..., mh, mw] over the header's tiles (32 x 32 from the origin, the last
    row / column of tiles takes what is left)"""
    mh, mw = m.shape[-2:]
    ty, tx = -(-mh // TILE), -(-mw // TILE)
    m = F.pad(m.double(), (0, tx * TILE - mw, 0, ty * TILE - mh))
    return m.reshape(m.shape[:-2] + (ty, TILE, tx, TILE)).sum((-3, -1))


def tile_pixels(mh, mw):
    """float64 [tiles_y, tiles_x]: the number of map pixels of each tile"""
    return tile_sums(torch.ones(mh, mw))


def table_of(tiles, sizes):
    """float64 [5,3,2] table of per-scale means from per-scale tile sums [3, 2, tiles_y, tiles_x]"""
    return np.stack([t.sum((-2, -1)).numpy() / ((h - 10) * (w - 10)) for t, (h, w) in zip(tiles, sizes)])


def score_of(table):
    """the score from a [5,3,2] table of means, float64: relu, weighted product over the scales, mean over the channels"""
    per_scale = np.concatenate([table[:4, :, 0], table[4:, :, 1]])
    return float(np.prod(np.maximum(per_scale, 0.0) ** np.asarray(WEIGHTS)[:, None], axis=0).mean())


def tile_cases():
    """(id, H, W, kind, silhouette) of the tile suite: every size of TILE_SIZES as noise and as texture or masked, the silhouette on
    one of the two; the two anticorrelated kinds at 161x178; the flagship frame once (the case of cases(), one reference for both)"""
    out = []
    for i, (H, W) in enumerate(TILE_SIZES):
        for kind, sil in (("noise", i % 2 == 1), (("texture", "masked")[i % 2], i % 2 == 0)):
            out.append(("%dx%d-%s-%s" % (H, W, kind, "sil" if sil else "nosil"), H, W, kind, sil))
    out.append(("161x178-anti-nosil", 161, 178, "anti", False))
    out.append(("161x178-anti1-nosil", 161, 178, "anti1", False))
    out.append(cases()[-1])
    return out


# the tile budget's factor on the fp32 restatement's own per-tile L1 distance from float64 (tests/test_gpu_msssim_tiles.py says where
# the figure comes from) and its floor per map pixel
TILE_M = 4.0
TILE_FLOOR = 1e-9
_tile_cache = {}


def tile_budget(l1, pixels):
    return TILE_M * l1 + TILE_FLOOR * pixels


def tile_reference(case):
    """of a case, computed once per session (callers must not modify it): dict of
      x, y       the masked float32 images
      levels64   [(x_s, y_s)] in float64
      tiles64    per scale float64 [3, 2, ty, tx]: tile sums of the float64 (cs, ssim) maps
      tiles32    the same of the float32 restatement's maps (summed in float64)
      l1         per scale [3, 2, ty, tx]: tile sums of |float32 restatement - float64|
      pixels     per scale [ty, tx]
      budget     per scale [3, 2, ty, tx]: tile_budget(l1, pixels)"""
    if case[0] not in _tile_cache:
        im, gt, depth, opacity, thres = reference(case)[:5]
        x, y = masked(im, gt, depth, opacity if case[4] else None, thres)
        ref = dict(x=x, y=y, levels64=levels(x, y, torch.float64), tiles64=[], tiles32=[], l1=[], pixels=[], budget=[])
        for m64, m32 in zip(scale_maps(x, y, torch.float64), scale_maps(x, y, torch.float32)):
            m64, m32 = torch.stack(m64, 1), torch.stack(m32, 1)
            ref["tiles64"].append(tile_sums(m64))
            ref["tiles32"].append(tile_sums(m32))
            ref["l1"].append(tile_sums((m32.double() - m64).abs()))
            ref["pixels"].append(tile_pixels(*m64.shape[-2:]))
            ref["budget"].append(tile_budget(ref["l1"][-1], ref["pixels"][-1]))
        _tile_cache[case[0]] = ref
    return _tile_cache[case[0]]
