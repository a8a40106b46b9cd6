"""-m gpu: the backward tile kernel's line-0 merge (hsr_render_bwd_q.hip, MERGE) against the CPU oracle.

With two channel groups and classic rows (K = 21..27) columns 0..6 of a splat's gradient row are summed over the tile's four quadrants in a
per-batch LDS table and leave once per (splat, tile) when the batch is over; K = 12 (compact rows) runs the per-quadrant emission and is
held to the same comparisons.  The scenes are hand-placed on one or two 16x16 tiles so that each path of the merge is taken on purpose:
a splat in four, two and one quadrant(s), a splat with a row in each of two tiles, slots reused and cleared over three batches with the last
batch sent after the loop, waves that skip whole batches while the others add, the median-depth gradient (column 6) on its own, and
partial tiles.  Tolerances: harness.assert_close (1e-4, tensor-wide and element-wise) plus the oracle's tie bound, as everywhere."""
import numpy as np
import pytest
import torch

import scenes
from harness import assert_close, run_gpu, run_oracle, tie_allowance
from hsr_utils.camera import replica_intrinsics, setup_camera_tensors
from hsr_utils.synthetic import make_upstream_grads

pytestmark = pytest.mark.gpu

KS = [12, 26, 27]
BATCH = 224   # splats staged per batch by the K >= 12 instantiations


def _scene(W, H, K, splats, seed=3):
    """splats: rows of (u, v, z, sigma_x, sigma_y, opacity) in pixels (u, v: image coordinates, a pixel's centre at i + 0.5; sigma: of the
    projected Gaussian before the rasterizer's 0.3 px^2 low-pass) -> camera at the origin, axis-aligned ellipsoids."""
    k = replica_intrinsics(W, H)
    cam = setup_camera_tensors(W, H, k, np.eye(4))
    s = torch.tensor(np.asarray(splats, np.float64))
    u, v, z, sx, sy, op = s.T
    fx, fy, cx, cy = k[0][0], k[1][1], k[0][2], k[1][2]
    means = torch.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    scales = torch.stack([sx * z / fx, sy * z / fy, 0.5 * (sx * z / fx + sy * z / fy)], 1)
    P = len(splats)
    g = torch.Generator(device="cpu").manual_seed(seed)
    rots = torch.zeros(P, 4)
    rots[:, 0] = 1.0
    sc = dict(means3D=means.float().contiguous(), scales=scales.float().contiguous(), rotations=rots.contiguous(),
              opacities=op.float().reshape(P, 1).contiguous(), colors_precomp=torch.rand(P, 3, generator=g).contiguous(),
              semantics_precomp=torch.rand(P, K, generator=g).contiguous())
    return cam, sc


def _upstream(W, H, K, only=None, positive=False):
    """positive: |N(0, 1)| per pixel.  A scene of one to four splats has gradient tensors of one to four rows, so the scale the 1e-4 bar
    refers to is a single splat's own sum over its pixels; with signed upstream gradients such a sum (dL_dopacity of a lone splat) can
    cancel to 1e-4 of its terms, and the bar would then measure the arrival order of fp32 atomics, not the kernel."""
    up = {n: v * float(W * H) for n, v in make_upstream_grads(W, H, K, seed=1).items()}   # O(1) per pixel: errors read as relative
    if positive:
        up = {n: v.abs() for n, v in up.items()}
    if only is not None:
        up = {n: (v if n == only else torch.zeros_like(v)) for n, v in up.items()}
    return up


CENTRE = [(8.0, 8.0, 2.0, 2.5, 2.5, 0.8)]                                   # on the tile's centre: all four quadrants
STRADDLE = [(8.0, 3.0, 2.5, 1.0, 1.0, 0.8), (3.0, 8.0, 3.0, 1.0, 1.0, 0.8)]   # over the vertical / the horizontal quadrant boundary: two quadrants each
SINGLE = [(14.0, 14.0, 1.5, 0.4, 0.4, 0.8)]                                 # inside sub-block (3, 3) of the tile


def _many(n, seed, opacity, z0=2.0, u_range=(0.0, 16.0)):
    r = np.random.RandomState(seed)
    return [(r.uniform(*u_range), r.uniform(0.0, 16.0), z0 + 4.0 * (i + r.uniform(0.2, 0.8)) / n, r.uniform(2.0, 3.5), r.uniform(2.0, 3.5), opacity)
            for i in range(n)]


def three_batches():
    """600 faint splats all over one tile: nobody's transmittance runs out, so the tile's list is three batches deep"""
    return _many(600, 5, 0.012)


def skip_path():
    """40 opaque splats in front over the left half only (tall, 2.5 px wide, centred on columns 1..5), 460 faint ones behind them"""
    r = np.random.RandomState(6)
    front = [(r.uniform(1.0, 5.0), 8.0, 1.0 + 0.01 * i, 2.5, 8.0, 0.99) for i in range(40)]
    return front + _many(460, 7, 0.012)


ONE_TILE = {"centre": CENTRE, "straddle": STRADDLE, "single": SINGLE, "all": CENTRE + STRADDLE + SINGLE}


def _check(cam, sc, up, want_state=False):
    out_g, gr_g, st_g = run_gpu(cam, sc, up, semantic=True, want_state=want_state)
    out_o, gr_o, st_o = run_oracle(cam, sc, up, semantic=True)
    try:
        assert st_o.bounds_info["overflow_pixels"] == 0, st_o.bounds_info
        for n in ("color", "depth", "opacity", "semantic"):
            assert_close(n, out_g[n], out_o[n], allowance=tie_allowance(n, st_o, out_g[n].shape, "pixel"))
        for n in gr_o:
            assert_close("grad " + n, gr_g[n], gr_o[n], allowance=tie_allowance("grad " + n, st_o, gr_g[n].shape, "gauss"))
        return st_g, np.asarray(st_o.field("n_contrib")).copy(), gr_o
    finally:
        st_o.free()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", list(ONE_TILE))
def test_one_tile_four_two_and_one_quadrant(name, K):
    cam, sc = _scene(16, 16, K, ONE_TILE[name])
    _, _, gr_o = _check(cam, sc, _upstream(16, 16, K, positive=True))
    assert all(np.abs(gr_o["means3D"][i]).max() > 0 for i in range(len(ONE_TILE[name]))), "a splat of the scene reaches no pixel"


@pytest.mark.parametrize("K", KS)
def test_a_splat_across_two_tiles_has_a_row_in_each(K):
    cam, sc = _scene(32, 16, K, [(16.0, 8.0, 2.0, 2.0, 2.0, 0.8), (5.0, 5.0, 3.0, 1.5, 1.5, 0.6), (27.0, 11.0, 3.5, 1.5, 1.5, 0.6)])
    _check(cam, sc, _upstream(32, 16, K, positive=True))


@pytest.mark.parametrize("only", [None, "median", "depth"])
@pytest.mark.parametrize("K", KS)
def test_three_batches_reuse_the_slots_and_the_last_batch_leaves_after_the_loop(K, only):
    cam, sc = _scene(16, 16, K, three_batches())
    _, n_contrib, gr_o = _check(cam, sc, _upstream(16, 16, K, only))
    assert n_contrib.max() > 2 * BATCH, "the scene no longer fills three batches: %d" % n_contrib.max()
    if only is not None:
        assert np.abs(gr_o["means3D"]).max() > 0


@pytest.mark.parametrize("K", KS)
def test_waves_that_skip_a_batch_add_nothing_and_are_not_waited_for(K):
    cam, sc = _scene(16, 16, K, skip_path())
    _, n_contrib, _ = _check(cam, sc, _upstream(16, 16, K))
    n = n_contrib.reshape(16, 16)
    hi_all = int(n.max())
    assert hi_all > 2 * BATCH, hi_all
    # the left quadrants' pixels all stop inside the front batch, so their waves skip the two batches behind it; the right ones do not
    assert n[:, :8].max() <= hi_all - 2 * BATCH, (int(n[:, :8].max()), hi_all)
    assert n[:8, 8:].max() == hi_all or n[8:, 8:].max() == hi_all


@pytest.mark.parametrize("only", ["median", "depth"])
@pytest.mark.parametrize("K", KS)
def test_column_6_arrives_once_per_splat(K, only):
    """upstream gradient on the median depth alone, then on the depth alone: whatever reaches dL_dmeans3D went through column 6 (K >= 21:
    the depth's direct sum has a column of its own, the median's does not) — a line sent twice, or never, is a factor 2, or 0"""
    cam, sc = _scene(16, 16, K, ONE_TILE["all"])
    _, _, gr_o = _check(cam, sc, _upstream(16, 16, K, only, positive=True))
    assert np.abs(gr_o["means3D"]).max() > 0


@pytest.mark.parametrize("K", KS)
def test_partial_tiles(K):
    cam, sc, up = scenes.build(40, 24, 200, K, seed=4, kind="aniso", scale_mult=2.0)
    _check(cam, sc, up)
