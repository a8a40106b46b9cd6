"""GPU suite for hsr_utils.slam.resample_frame / hsr_frame_resample (include/ext/hsr_frame_resample.h) against the two float64
restatements of tests/resample_ref.py (which tests/test_slam_multires_cpu.py shows to agree to 1e-12).

Colour is uniform in [0, 1) and must lie within 1e-6 of the float64 references: the kernel's value is three lerps a + f * (b - a),
eight fp32 roundings of values <= 1 at 6e-8 each, hence at most 5e-7 (an fp32 restatement on the CPU measured 1.4e-7).  Depth carries
a block of zeros, one NaN and one inf and must be bit-equal to the references, compared as int32 over every pixel.  The largest colour
distance of every case is printed (the first MI355X run's figures are in profiles/multires_gpu.log)."""
import functools

import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu

COLOUR_TOL = 1e-6
IDS = ["%dx%d-%dx%d" % (s + d) for s, d in R.SIZE_PAIRS]
# two levels of one call: the 97x130 frame to 48x64 and to 18x11 (the size 37x23 is reduced to); odd to two odd sizes; up and identity
TWO_LEVELS = (((97, 130), ((48, 64), (18, 11))), ((37, 23), ((18, 11), (19, 12))), ((48, 64), ((97, 130), (48, 64))))


@functools.lru_cache(maxsize=None)
def _frame(src):
    color, depth = R.make_frame(*src, seed=100 * src[0] + src[1])
    return color, depth, color.cuda(), depth.cuda()[None]


@functools.lru_cache(maxsize=None)
def _reference(src, dst):
    color, depth, _c, _d = _frame(src)
    return R.resample_torch(color, depth, dst), R.resample_scipy(color, depth, dst)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(src, dst, got_color, got_depth):
    (ct, dt), (cs, ds) = _reference(src, dst)
    assert got_color.shape == (3,) + dst and got_depth.shape == (1,) + dst
    assert got_color.dtype == got_depth.dtype == torch.float32 and got_color.is_contiguous() and got_depth.is_contiguous()
    gc, gd = got_color.cpu(), got_depth.cpu()[0]
    dist = max(float((gc.double() - ct).abs().max()), float((gc.double() - cs).abs().max()))
    assert torch.equal(_bits(gd), _bits(dt)) and torch.equal(_bits(gd), _bits(ds))      # every pixel, NaN and inf included
    return dist


@pytest.mark.parametrize("src,dst", R.SIZE_PAIRS, ids=IDS)
def test_one_level_matches_float64(src, dst):
    from hsr_utils import resample_frame
    color, depth, color_d, depth_d = _frame(src)
    (got_color, got_depth), = resample_frame(color_d, depth_d, [dst])
    dist = _check(src, dst, got_color, got_depth)
    print("frame_resample %dx%d -> %dx%d: largest colour distance from float64 %.3g" % (src + dst + (dist,)))
    assert dist <= COLOUR_TOL
    if src == dst:      # fx = fy = 0: a copy, bit for bit
        assert torch.equal(_bits(got_color.cpu()), _bits(color)) and torch.equal(_bits(got_depth.cpu()[0]), _bits(depth))
    if (src, dst) == ((16, 16), (8, 8)):      # exact 2x: the 2x2 mean, and every second depth
        mean = color.double().reshape(3, 8, 2, 8, 2).mean(dim=(2, 4))
        assert float((got_color.cpu().double() - mean).abs().max()) <= COLOUR_TOL
        assert torch.equal(_bits(got_depth.cpu()[0]), _bits(depth[::2, ::2]))
    again = resample_frame(color_d, depth_d, [dst])[0]      # two calls are bit-identical
    assert torch.equal(_bits(again[0]), _bits(got_color)) and torch.equal(_bits(again[1]), _bits(got_depth))


@pytest.mark.parametrize("src,dsts", TWO_LEVELS, ids=["%dx%d" % s for s, _ in TWO_LEVELS])
def test_two_levels_equal_two_one_level_calls(src, dsts):
    from hsr_utils import resample_frame
    _color, _depth, color_d, depth_d = _frame(src)
    both = resample_frame(color_d, depth_d, list(dsts))
    assert len(both) == 2
    for dst, (got_color, got_depth) in zip(dsts, both):
        (one_color, one_depth), = resample_frame(color_d, depth_d, [dst])
        assert torch.equal(_bits(got_color), _bits(one_color)) and torch.equal(_bits(got_depth), _bits(one_depth))
        dist = _check(src, dst, got_color, got_depth)
        print("frame_resample %dx%d -> %dx%d (of two levels): largest colour distance from float64 %.3g" % (src + dst + (dist,)))
        assert dist <= COLOUR_TOL


def test_one_level_call_writes_nothing_else():
    """the C entry point with H1 == 0 and a guard-filled second pair of buffers, and guard words behind level 0's outputs"""
    from diff_gaussian_rasterization import _abi
    src, dst = (37, 23), (19, 12)
    _color, _depth, color_d, depth_d = _frame(src)
    n, guard, fill = dst[0] * dst[1], 64, -7.25
    out_c = torch.full((3 * n + guard,), fill, device="cuda")
    out_d = torch.full((n + guard,), fill, device="cuda")
    second_c, second_d = torch.full((3 * n,), fill, device="cuda"), torch.full((n,), fill, device="cuda")
    _abi.call(_abi.lib.hsr_frame_resample, "hsr_frame_resample", color_d.device, src[0], src[1], color_d.data_ptr(), depth_d.data_ptr(),
              dst[0], dst[1], out_c.data_ptr(), out_d.data_ptr(), 0, dst[1], second_c.data_ptr(), second_d.data_ptr())
    assert bool((second_c == fill).all()) and bool((second_d == fill).all())
    assert bool((out_c[3 * n:] == fill).all()) and bool((out_d[n:] == fill).all())
    assert _check(src, dst, out_c[:3 * n].reshape(3, *dst), out_d[:n].reshape(1, *dst)) <= COLOUR_TOL


def test_non_contiguous_input():
    from hsr_utils import resample_frame
    src, dsts = (33, 65), [(17, 33), (40, 70)]
    _color, _depth, color_d, depth_d = _frame(src)
    hwc = color_d.permute(1, 2, 0).contiguous().permute(2, 0, 1)                      # [3,H,W] strides of an [H,W,3] image
    wide = torch.zeros(1, src[0], 2 * src[1], device="cuda")
    wide[..., ::2] = depth_d
    assert not hwc.is_contiguous() and not wide[..., ::2].is_contiguous()
    for (a_c, a_d), (b_c, b_d) in zip(resample_frame(hwc, wide[..., ::2], dsts), resample_frame(color_d, depth_d, dsts)):
        assert torch.equal(_bits(a_c), _bits(b_c)) and torch.equal(_bits(a_d), _bits(b_d))
    (c, d), = resample_frame(color_d, depth_d[0], [dsts[0]])                             # a [H,W] depth is taken too
    assert _check(src, dsts[0], c, d) <= COLOUR_TOL


def test_refusals_launch_nothing(monkeypatch):
    from hsr_utils import resample_frame, slam
    calls = []
    real = slam._lib.hsr_frame_resample
    monkeypatch.setattr(slam._lib, "hsr_frame_resample", lambda *a: calls.append(a) or real(*a))
    _color, _depth, color_d, depth_d = _frame((5, 7))
    with pytest.raises(RuntimeError, match="no CPU path"):
        resample_frame(color_d.cpu(), depth_d.cpu(), [(2, 3)])
    with pytest.raises(RuntimeError, match="no CPU path"):
        resample_frame(color_d, depth_d.cpu(), [(2, 3)])
    for bad in ([(0, 3)], [(2, 0)], [(16385, 3)], [(2, 3), (2, 16385)], [], [(2, 3)] * 3):
        with pytest.raises(ValueError, match="resample_frame"):
            resample_frame(color_d, depth_d, bad)
    with pytest.raises(RuntimeError, match=r"color must be \[3,H,W\]"):
        resample_frame(torch.zeros(4, 5, 7, device="cuda"), depth_d, [(2, 3)])
    with pytest.raises(RuntimeError, match=r"color must be \[3,H,W\]"):
        resample_frame(color_d, torch.zeros(1, 5, 8, device="cuda"), [(2, 3)])
    assert calls == []
    resample_frame(color_d, depth_d, [(2, 3)])
    assert len(calls) == 1                                                              # the wrapper does see a launch
