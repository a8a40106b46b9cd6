"""Depth / gt pairs at the edges of an exact median of the depth error |gt - d| * (gt > 0): the inputs of the two device selects that compute it,
hsr_loss_outlier_median (include/ext/hsr_loss_outlier.h: three passes of 11, 11 and 10 bits) and the select of hsr_densify_frame
(include/hsr_densify.h: four passes of 8 bits, most significant byte first, 2048 values per workgroup, one mask block per 256 pixels).

    CASES            the loss head's table (tests/test_gpu_loss_outlier.py runs exactly these)
    DENSIFY_CASES    the cases that belong to the 8-bit select and to the densify mask
    ALL_CASES        both; tests/test_densify_frame_cases_cpu.py holds every one to the regime it is named for, tests/test_gpu_densify_frame_edges.py
                     runs every one through both selects

Every builder returns (depth, gt): the rendered depth and the measured one, fp32 [H,W] CPU tensors."""
import torch

NAN, INF = float("nan"), float("inf")


def _noisy(H, W, seed, holes=0.1, outliers=0.05):
    """gt depth 0.5..5 m with holes, a rendered depth = gt + Gaussian noise (sigma 1 cm), `outliers` of the pixels 50 times noisier"""
    g = torch.Generator().manual_seed(seed)
    gt = 0.5 + 4.5 * torch.rand(H, W, generator=g)
    noise = 0.01 * torch.randn(H, W, generator=g)
    noise = torch.where(torch.rand(H, W, generator=g) < outliers, 50 * noise, noise)
    depth = gt + noise
    gt = torch.where(torch.rand(H, W, generator=g) < holes, torch.zeros(()), gt)
    return depth, gt


def _from_errors(errors, shape, holes=0, seed=0, hole_depth=1.0):
    """depth 0 and gt = the given errors (so that e = gt exactly), shuffled, then `holes` pixels of gt = 0 under a depth of hole_depth"""
    g = torch.Generator().manual_seed(seed)
    e = torch.as_tensor(errors, dtype=torch.float32)
    n = shape[0] * shape[1]
    assert e.numel() + holes == n
    gt = torch.cat([e, torch.zeros(holes)])
    depth = torch.cat([torch.zeros(e.numel()), torch.full((holes,), hole_depth)])
    perm = torch.randperm(n, generator=g)
    return depth[perm].reshape(shape).contiguous(), gt[perm].reshape(shape).contiguous()


def _with(pair, **cells):
    """a case with single cells replaced: d_IJ = value / g_IJ = value for depth / gt at row I, column J"""
    depth, gt = pair[0].clone(), pair[1].clone()
    for key, v in cells.items():
        t = depth if key[0] == "d" else gt
        i, j = (int(x) for x in key[2:].split("_"))
        t[i, j] = v
    return depth, gt


def _small():      # 3 x 5, every pixel valid, errors 0.1 .. 1.5
    gt = torch.arange(1, 16, dtype=torch.float32).reshape(3, 5) * 0.25 + 1.0
    return gt - 0.1 * torch.arange(1, 16, dtype=torch.float32).reshape(3, 5), gt


_DEN = 2.0 ** -149      # the smallest fp32 denormal
CASES = {
    # one pixel: selected; a hole: median 0, nothing is < 0, the mean of nothing is NaN
    "1x1_valid": lambda: (torch.tensor([[1.5]]), torch.tensor([[2.0]])),
    "1x1_hole": lambda: (torch.tensor([[1.5]]), torch.tensor([[0.0]])),
    # e = {1, 20}: the lower median 1 selects one pixel, an upper median would select both; the same on 2 x 2
    "1x2_lower_median": lambda: (torch.zeros(1, 2), torch.tensor([[1.0, 20.0]])),
    "2x2_lower_median": lambda: (torch.zeros(2, 2), torch.tensor([[1.0, 20.0], [20.0, 1.0]])),
    # n = 35, rank 17: 18 zeros reach it (median 0, empty selection); 17 do not (the smallest positive error, 0.05, is the median)
    "5x7_18_holes": lambda: _from_errors([0.05 + 0.07 * k for k in range(17)], (5, 7), holes=18, seed=1),
    "5x7_17_holes": lambda: _from_errors([0.05 + 0.07 * k for k in range(18)], (5, 7), holes=17, seed=2),
    # every valid pixel has the error 0.5 (2.0 - 1.5, exact): all of them are selected
    "equal_errors": lambda: (torch.full((9, 13), 1.5), torch.where(torch.arange(117).reshape(9, 13) % 4 == 0, 0.0, 2.0)),
    # keys that differ only in the bits of the last pass (9..0), and only in those of the middle pass (20..10)
    "32x32_last_pass": lambda: _from_errors([1.0 + k * 2.0 ** -23 for k in range(1024)], (32, 32), seed=3),
    "32x32_middle_pass": lambda: _from_errors([1.0 + k * 2.0 ** -13 for k in range(1024)], (32, 32), seed=4),
    # median 0.5, threshold 5.0, one pixel at exactly 5.0: the strict < excludes it
    "tie_at_threshold": lambda: _from_errors([0.5] * 5 + [5.0, 0.25, 0.25, 7.0], (3, 3), seed=5),
    # denormal errors (a denormal gt against depth 0): median 311000 * 2^-149, four pixels beyond ten times it
    "denormal_errors": lambda: _from_errors([(300000 + 1000 * k) * _DEN for k in range(16)] + [m * _DEN for m in (
        2000000, 2400000, 2800000, 3100000, 3110000, 4000000, 6000000, 8388607)], (4, 6), seed=6),
    # NaN and inf depth: a NaN error anywhere makes the median NaN and the selection empty; an inf error on a valid pixel only drops out
    "nan_depth_valid_pixel": lambda: _with(_small(), d_1_2=NAN),
    "nan_depth_under_hole": lambda: _with(_small(), d_1_2=NAN, g_1_2=0.0),
    "inf_depth_under_hole": lambda: _with(_small(), d_2_4=INF, g_2_4=0.0),
    "inf_depth_valid_pixel": lambda: _with(_small(), d_0_3=INF),
    # a negative gt is a hole: its error is 0 and it is never selected
    "negative_gt": lambda: _with(_small(), g_0_0=-1.0, g_1_1=-0.5, g_2_2=-3.0, g_2_3=0.0),
    # tails of a wave and of a workgroup; several workgroups
    "37x23": lambda: _noisy(37, 23, seed=7),
    "129x67": lambda: _noisy(129, 67, seed=8),
    # many workgroups, a non-trivial bin in all three passes
    "340x600": lambda: _noisy(340, 600, seed=9, holes=0.03),
    # one partial per 1024 pixels; the finish kernel's 256 threads take a second trip from 257 partials on: H * W > 256 * 1024 = 262 144
    "513x512": lambda: _noisy(513, 512, seed=10),
    # the outlier head's grid stops at 512 workgroups and strides from H * W > 512 * 1024 = 524 288 on (the plain head's does not stop)
    "725x724": lambda: _noisy(725, 724, seed=11),
}


# ---- the densify select: four passes of 8 bits (byte 3 first), 2048 values per histogram workgroup, 256 pixels per mask block ----------
def _from_bits(bits, shape, seed):
    """errors given as fp32 bit patterns (all finite and non-negative), through _from_errors"""
    e = torch.tensor(list(bits), dtype=torch.int32).view(torch.float32)
    return _from_errors(e, shape, seed=seed)


def _bucket_255(median_bits, below, above, seed):
    """nine errors: five copies of median_bits, two below, two above: ranks 2 .. 6 are the copies, rank 4 is the median"""
    return _from_bits(list(below) + [median_bits] * 5 + list(above), (3, 3), seed)


def _nan_turns_the_depth_mask_off():
    """errors {NaN, 0, 0, e, e, e, 1} with e = 2^-10, all of them with rendered > gt: the rank-3 element is e, and 1 > 50 e would select the last
    pixel; torch's median is NaN and selects nothing.  The NaN is inf * 0: an infinite rendered depth over a hole"""
    e = 2.0 ** -10
    gt = torch.tensor([[0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]])
    return torch.tensor([[INF, 1.0 + e, 1.0 + e, 1.0 + e, 1.0, 1.0, 2.0]]), gt


def _nan_in_the_last_workgroup():
    """2049 pixels: the second histogram workgroup holds one pixel, and its error is NaN"""
    depth, gt = _noisy(3, 683, seed=16, holes=0.0)
    depth[2, 682] = NAN
    return depth, gt


DENSIFY_CASES = {
    # one case per byte: keys that differ in that byte alone, so three passes see one occupied bucket and one pass sees them all
    "byte0_only": lambda: _from_bits([0x3f800000 + k for k in range(256)], (16, 16), 20),
    "byte1_only": lambda: _from_bits([0x3f800000 + (k << 8) for k in range(256)], (16, 16), 21),
    "byte2_only": lambda: _from_bits([0x3f000000 + (k << 16) for k in range(256)], (16, 16), 22),
    "byte3_only": lambda: _from_bits([k << 24 for k in range(128)], (8, 16), 23),      # 0 .. 2^127; the median's top byte is 63
    # the rank falls in bucket 255 of the last, the third and the second pass: the end of the pick loop
    "bucket255_byte0": lambda: _bucket_255(0x3f8000ff, (0x3f800000, 0x3f800010), (0x3f800100, 0x3f800200), 24),
    "bucket255_byte1": lambda: _bucket_255(0x3f80ff80, (0x3f800000, 0x3f801000), (0x3f810000, 0x3f820000), 25),
    "bucket255_byte2": lambda: _bucket_255(0x3fff0000, (0x3f000000, 0x3f100000), (0x40000000, 0x40100000), 26),
    # 8 of 15 errors are +inf on valid pixels: median inf, threshold inf, nothing is greater
    "mostly_inf_errors": lambda: _with(_small(), d_0_0=INF, d_0_2=INF, d_0_4=INF, d_1_1=INF, d_1_3=INF, d_2_0=INF, d_2_2=INF, d_2_4=INF),
    # NaN errors: from a NaN gt; the worked example (median 0.1 by rank, NaN by torch); one that decides a pixel; one counted by the last workgroup
    "nan_gt": lambda: _with(_small(), g_1_2=NAN),
    "1x7_inf_over_hole": lambda: (torch.tensor([[INF, 1.1, 2.1, 3.0, 4.5, 9.0, 6.0]]), torch.tensor([[0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0]])),
    "nan_turns_depth_mask_off": _nan_turns_the_depth_mask_off,
    "3x683_nan_last_pixel": _nan_in_the_last_workgroup,
    # H * W around the 2048 values of a histogram workgroup
    "23x89": lambda: _noisy(23, 89, seed=12),       # 2047
    "32x64": lambda: _noisy(32, 64, seed=13),       # 2048
    "3x683": lambda: _noisy(3, 683, seed=14),       # 2049
    # exactly 1024 mask blocks: one count per thread of the scan; "513x512" of CASES has 1026: two counts per thread
    "512x512": lambda: _noisy(512, 512, seed=15),
}
assert not set(CASES) & set(DENSIFY_CASES)
ALL_CASES = {**CASES, **DENSIFY_CASES}


# ---- whole densify frames: silhouette, rendered depth, gt depth, colour, intrinsics, w2c (fp32 CPU tensors) ------------------------------
SIL_THRES = 0.5


def _camera(H, W):
    """the pinhole and the tilted pose of tests/test_densify.make_frame at this size"""
    from test_densify import make_frame
    K, w2c = make_frame(2, 2, 0)[4:]
    K = K.copy()
    K[0, 0] = K[1, 1] = W * 0.5
    K[0, 2], K[1, 2] = W / 2 - 0.5, H / 2 - 0.5
    return torch.tensor(K), torch.tensor(w2c)


def _frame(sil, rd, gt, seed):
    H, W = gt.shape
    col = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1000 + seed))
    return (sil.contiguous(), rd.contiguous(), gt.contiguous(), col) + _camera(H, W)


def densify_frame(case):
    """a case of ALL_CASES as a densify frame.  Up to 16 pixels the silhouette is 1 everywhere, so the mask is its depth part alone; larger
    frames have a silhouette of 0.9 .. 1 with an eighth of the pixels (a run of the flat index) at 0.1"""
    rd, gt = ALL_CASES[case]()
    N = gt.numel()
    if N <= 16:
        sil = torch.ones_like(gt)
    else:
        sil = 0.9 + 0.1 * torch.rand(gt.shape, generator=torch.Generator().manual_seed(500 + len(case)))
        sil.view(-1)[N // 3: N // 3 + N // 8] = 0.1
    return _frame(sil, rd, gt, len(case))


def comparison_frame(depth_factor, nan_gt=False):
    """16 pixels that sit on every comparison of the mask, and the mask they must give.  gt = 1 and rendered = 1 + k e with e = 2^-10 (or
    2^-11 steps for the threshold pair), so every error is exact; ten errors are e, three are 0: the median is e and the threshold is
    depth_factor * e, exact for 50 and for 12.5.
       7   error == threshold, rendered > gt                 out (strict >)
       8   error == threshold + 2^-11, rendered > gt         IN
       6   rendered == gt (error 0)                          out
       9   error 0.5 but rendered < gt                       out
      10   silhouette == sil_thres                           out (strict <)
      11   silhouette one ulp under sil_thres                IN
      12   silhouette NaN                                    out
      13   gt 0, 14 gt -1: silhouette 0.1, error 0           out
      15   nan_gt: gt NaN under a silhouette of 0.1: out, and its NaN error turns the median NaN, which puts pixel 8 out as well"""
    e, thr = 2.0 ** -10, depth_factor * 2.0 ** -10
    gt, rd, sil = torch.ones(16), torch.full((16,), 1.0 + e), torch.ones(16)
    rd[6], rd[7], rd[8], rd[9] = 1.0, 1.0 + thr, 1.0 + thr + 2.0 ** -11, 0.5
    sil[10], sil[11], sil[12] = SIL_THRES, float(torch.nextafter(torch.tensor(SIL_THRES), torch.tensor(0.0))), NAN
    gt[13], gt[14] = 0.0, -1.0
    sil[13] = sil[14] = 0.1
    want = [8, 11]
    if nan_gt:
        gt[15], sil[15], want = NAN, 0.1, [11]
    expect = torch.zeros(16, dtype=torch.bool)
    expect[want] = True
    return _frame(sil.reshape(2, 8), rd.reshape(2, 8), gt.reshape(2, 8), 7), expect


EMISSION_MASKS = ("edges", "everywhere", "nowhere")


def emission_frame(which):
    """3 x 100 pixels, every depth valid and rendered == gt (median 0, no depth part): the silhouette alone sets the mask, at the last lane of a
    wave, the first of the next, the last thread of a block, the first of the next and the last pixel; everywhere; nowhere"""
    H, W = 3, 100
    g = torch.Generator().manual_seed(77)
    gt = 0.5 + 4.5 * torch.rand(H, W, generator=g)
    sil = torch.ones(H, W)
    if which == "edges":
        sil.view(-1)[[63, 64, 255, 256, H * W - 1]] = 0.1
    elif which == "everywhere":
        sil.fill_(0.1)
    return _frame(sil, gt.clone(), gt, 8)
