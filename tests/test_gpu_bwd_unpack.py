"""-m gpu: the backward's unpack of the packed gradient rows (hsr_backward_pre.hip, preprocess_backward_kernel) against the CPU oracle.

The kernel brings a block's 256 rows into LDS in passes of whole rows (16-byte loads, each 64-byte line requested once), writes the block's
[256, K] piece of dL_dsemantics from there — 16 bytes per lane where the piece is 16-byte aligned, dwords otherwise — and hands each lane its
own columns.  What can go wrong is in the seams: the last, partial block and pass, every row stride and both row layouts, culled rows
(never zero-filled, never to be read) between visible ones, destinations at 4-byte offsets (the gradient sink), and the optional outputs.
Tolerances: harness.assert_close (1e-4, tensor-wide and element-wise) plus the oracle's tie bound, as everywhere.

Scenes: kind "slam" — isotropic Gaussians, what a SLAM map holds and what bench.py runs.  With them the conic -> cov3D -> scale chain
behind the unpack is well-conditioned, so the 1e-4 bar measures what the kernel moved; on needles an entry of that chain sits at 1-3e-4 of
the bar from one run to the next with the arrival order of the tile kernel's fp32 atomics (harness.FLOOR_FRAC_COV), whatever the unpack
does.  That chain's arithmetic is not what this file is about: test_gpu_gauss_chain.py holds it, bit for bit, to the oracle's chain run on the
device's own accumulated sums (needles, clamped and culled Gaussians, every input variant), where the arrival order drops out."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scenes
from harness import _cam_to, assert_close, run_gpu, run_oracle, tie_allowance

pytestmark = pytest.mark.gpu

W, H = 64, 48
LEAVES = ("means3D", "opacities", "colors_precomp", "scales", "rotations", "semantics_precomp")


def _against_oracle(cam, sc, up, gr_g, out_g=None, semantic=True, variant="sr", extra=None):
    out_o, gr_o, st_o = run_oracle(cam, sc, up, semantic=semantic, variant=variant, extra=extra)
    try:
        assert st_o.bounds_info["overflow_pixels"] == 0, st_o.bounds_info
        if out_g is not None:
            for n in ("color", "depth", "opacity") + (("semantic",) if semantic else ()):
                assert_close(n, out_g[n], out_o[n], allowance=tie_allowance(n, st_o, out_g[n].shape, "pixel"))
        for n in gr_o:
            assert n in gr_g, n
            assert_close("grad " + n, gr_g[n], gr_o[n], allowance=tie_allowance("grad " + n, st_o, gr_g[n].shape, "gauss"))
        return out_o, gr_o
    finally:
        st_o.free()


def _check(cam, sc, up, semantic=True, variant="sr", extra=None):
    out_g, gr_g, _ = run_gpu(cam, sc, up, semantic=semantic, variant=variant, extra=extra, want_state=False)
    _against_oracle(cam, sc, up, gr_g, out_g, semantic, variant, extra)
    return out_g, gr_g


@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 511, 513, 1300])
def test_p_at_the_block_and_pass_seams(P):
    """K = 26: 48-float rows, two passes of 128 rows per block — a block of one row, a wave more or less, a pass more or less, a block more
    or less, and 1300 = five blocks and 20 rows"""
    _check(*scenes.build(W, H, P, 26, seed=P, kind="slam", scale_mult=3.0))


# K -> (row layout, stride in floats) as the plan chooses them (tests/test_backward_plan.py)
LAYOUTS = {0: (1, 16), 5: (0, 32), 11: (0, 32), 12: (1, 32), 16: (1, 32), 20: (1, 32), 21: (0, 48), 26: (0, 48), 27: (0, 48),
           28: (0, 64), 53: (0, 80), 74: (0, 96), 102: (0, 128)}


@pytest.mark.parametrize("K", list(LAYOUTS))
def test_every_row_layout_and_stride_with_culled_rows_between_visible_ones(K):
    from diff_gaussian_rasterization import _abi
    import ctypes as C
    P = 600
    plan = _abi.hsr_backward_plan()
    assert _abi.lib.hsr_plan_backward(P, K, 0, _abi.HSR_SCRATCH_AS_PLANNED, C.byref(plan)) >= 0
    assert (int(plan.row_layout), int(plan.row_stride)) == LAYOUTS[K], "the plan's rows at K = %d are not what this test was written for" % K
    cam, sc, up = scenes.build(W, H, P, K, seed=7, kind="slam", scale_mult=3.0, behind_frac=0.3)
    out_g, _ = _check(cam, sc, up)
    culled = int((out_g["radii"] <= 0).sum())
    assert 0 < culled < P, culled


def _forward_poison_backward(cam, sc, up, K):
    """forward; then a NaN-filled tensor of the backward scratch's size (and one twice as large) is allocated and freed, so that the
    caching allocator is likely to hand the backward poisoned rows; then the backward"""
    from diff_gaussian_rasterization import GaussianRasterizer_semantic, _abi
    dev = torch.device("cuda:0")
    P = sc["means3D"].shape[0]
    leaf = {n: sc[n].to(dev).clone().requires_grad_(True) for n in LEAVES}
    means2D = torch.zeros(P, 3, device=dev, requires_grad=True)
    color, radii, sem, depth, median, opac = GaussianRasterizer_semantic(_cam_to(cam, dev))(means2D=means2D, **leaf)
    loss = (color * up["color"].to(dev)).sum() + (depth * up["depth"].to(dev)).sum() + (median * up["median"].to(dev)).sum() \
        + (opac * up["opacity"].to(dev)).sum()
    if K > 0:
        loss = loss + (sem * up["semantic"].to(dev)).sum()
    nbytes = int(_abi.lib.hsr_backward_scratch_bytes(P, K, 0))
    assert nbytes >= P * 16 * 4
    torch.cuda.synchronize()
    for n in (nbytes, 2 * nbytes):
        poison = torch.full((n // 4,), float("nan"), device=dev)
        torch.cuda.synchronize()
        del poison
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: v.grad.cpu().numpy() for n, v in leaf.items()}
    grads["means2D"] = means2D.grad.cpu().numpy()
    return radii.cpu().numpy(), grads


@pytest.mark.parametrize("behind", [0.5, 1.0])
@pytest.mark.parametrize("K", [0, 16, 26, 74])
def test_culled_rows_are_never_read(K, behind):
    P = 700
    cam, sc, up = scenes.build(W, H, P, K, seed=9, kind="slam", scale_mult=3.0, behind_frac=behind)
    if behind == 1.0:
        sc["means3D"][:, 2] = -torch.abs(sc["means3D"][:, 2]) - 1.0   # behind the camera for sure
    radii, grads = _forward_poison_backward(cam, sc, up, K)
    culled = radii <= 0
    assert culled.sum() >= (P if behind == 1.0 else P // 4), int(culled.sum())
    for n, g in grads.items():
        assert not np.isnan(g).any(), n
        assert np.isfinite(g).all(), n
        assert (g[culled] == 0.0).all(), "%s: a culled Gaussian has a gradient" % n
    if behind < 1.0:
        assert culled.sum() < P
        _against_oracle(cam, sc, up, grads)


class _OffsetSink:
    """a gradient sink whose tensors start `off` floats (4 * off bytes) into a buffer of sentinels"""
    SENTINEL, MARGIN = -12345.5, 8

    def __init__(self, off):
        self.off, self.bufs = off, {}

    def __call__(self, name, shape, dev):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * self.MARGIN,), self.SENTINEL, device=dev)
        assert buf.data_ptr() % 16 == 0
        self.bufs[name] = (buf, n)
        return buf[self.off:self.off + n].view(shape)

    def check(self, grads):
        assert {"raster." + n for n in LEAVES} <= set(self.bufs), sorted(self.bufs)
        for name, (buf, n) in self.bufs.items():
            b = buf.cpu().numpy()
            assert (b[:self.off] == self.SENTINEL).all(), "%s: floats in front of the view were written" % name
            assert (b[self.off + n:] == self.SENTINEL).all(), "%s: floats behind the view were written" % name
            key = name.replace("raster.", "")
            assert np.array_equal(b[self.off:self.off + n].reshape(grads[key].shape), grads[key]), "%s: the gradient is not what the view holds" % name


_ALIGNED = {}   # (K, P) -> (scene, gradients of the run without a sink)


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("P", [257, 600])
@pytest.mark.parametrize("K", [16, 26, 27])
def test_destinations_at_4_byte_offsets(K, P, off):
    from diff_gaussian_rasterization import _C
    if (K, P) not in _ALIGNED:
        cam, sc, up = scenes.build(W, H, P, K, seed=13, kind="slam", scale_mult=3.0, behind_frac=0.2)
        _, gr, _ = run_gpu(cam, sc, up, want_state=False)
        _ALIGNED[(K, P)] = (cam, sc, up, gr)
    cam, sc, up, aligned = _ALIGNED[(K, P)]
    sink = _OffsetSink(off)
    prev = _C.set_gradient_sink(sink)
    try:
        _, gr, _ = run_gpu(cam, sc, up, want_state=False)
    finally:
        _C.set_gradient_sink(prev)
    sink.check(gr)
    for n in aligned:
        assert_close("grad %s at byte offset %d" % (n, 4 * off), gr[n], aligned[n])


@pytest.mark.parametrize("K", [16, 26])
def test_geometry_only_backward(K):
    """only means3D / means2D require a gradient: 16-float rows, no colour, opacity or semantic output"""
    from test_gpu_parity import _pose_only_and_full_gradients
    cam, sc, up = scenes.build(W, H, 600, K, seed=15, kind="slam", scale_mult=3.0, behind_frac=0.3)
    grads = _pose_only_and_full_gradients(cam, sc, up, True)
    out_o, go, so = run_oracle(cam, sc, up)
    try:
        assert_close("means3D (geometry-only)", grads["pose"][0], go["means3D"], allowance=tie_allowance("grad means3D", so, go["means3D"].shape, "gauss"))
        assert_close("means2D (geometry-only)", grads["pose"][1], go["means2D"], allowance=tie_allowance("grad means2D", so, go["means2D"].shape, "gauss"))
    finally:
        so.free()


@pytest.mark.parametrize("semantic,K", [(True, 26), (False, 0)])
def test_precomputed_covariance_has_no_scale_or_rotation_output(semantic, K):
    cam, sc, up = scenes.build(W, H, 600, K, seed=17, kind="slam", scale_mult=3.0, behind_frac=0.3)
    _check(cam, sc, up, semantic=semantic, variant="cov", extra={"cov3D_precomp": scenes.cov3d_from_scene(sc)})


@pytest.mark.parametrize("deg", [0, 1])
def test_sh_colours(deg):
    P = 600
    cam, sc, up = scenes.build(W, H, P, 26, seed=19, kind="slam", scale_mult=3.0, behind_frac=0.3)
    cam["sh_degree"] = deg
    _check(cam, sc, up, extra={"shs": scenes.random_sh(P, 16)})


_CHILD = ("import sys; sys.path[:0]=['hier-slam_amd','tests']; import scenes, test_gpu_bwd_unpack as t;"
          "from diff_gaussian_rasterization import _C; _C.set_backward_mode(sys.argv[1]);"
          "[t._check(*scenes.build(64, 48, 600, K, seed=21, kind='slam', scale_mult=3.0, behind_frac=0.3)) for K in (26, 74)]; print('ok')")


@pytest.mark.parametrize("mode,impl", [("legacy", None), ("packed", "valu")])
def test_legacy_accumulation_and_the_valu_family_in_a_child_process(mode, impl):
    """the paths this kernel's packed mode does not serve (legacy: the sums arrive in the reference's arrays) or that fill its rows with
    another tile kernel (HSR_BWD_IMPL=valu, read once per process)"""
    env = dict(os.environ)
    env.pop("HSR_BWD_IMPL", None)
    if impl:
        env["HSR_BWD_IMPL"] = impl
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHILD, mode], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
