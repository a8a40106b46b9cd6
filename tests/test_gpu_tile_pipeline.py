"""-m gpu: the tile kernels' staging pipeline (hsr_render_fwd.hip, hsr_render_bwd_q.hip, hsr_bwd_tile.h) against the CPU oracle.

Both tile kernels keep the gathers of the next batch in flight while the current batch is blended and wait for them once, at the top of
the batch that stages them.  A wait that came too late, or stood on one path only, would stage a register whose load has not landed: a
wrong splat in a slot of some batch.  The scenes are the smallest at which that would show — one or two 16x16 tiles, lists of exactly
0, 1, B - 1, B, B + 1, 2 B and 2 B + 1 entries for the forward's batch of 240 and the backward's of 224 (one, two and three batches, a
last batch of one entry, a slot staged by three batches), waves that stop early and skip a batch (the forward's wave_done path, the
backward's `hi - cnt >= wmax`), a wave whose list is empty in the middle batch of three, every kernel variant, both launch paths of
the forward and a map with every fifth Gaussian culled.

Scenes are built as in tests/test_gpu_fwd_visit_loop.py: hand-placed, and free of tie-risk pixels in the oracle (asserted), so n_contrib
and median_pos are compared exactly on every pixel.  Images and gradients: harness.assert_close at its tolerances (1e-4, tensor-wide
and element-wise) plus the oracle's tie bound, which is zero here.  Radii, the sorted lists and the tile ranges: bit-equal."""
import os

import numpy as np
import pytest
import torch

from harness import assert_close, run_gpu, run_oracle, tie_allowance
from test_gpu_fwd_visit_loop import _depths, _many, _scene, _upstream

pytestmark = pytest.mark.gpu

FWD_BATCH = {0: 240, 16: 240, 26: 240, 27: 200, 5: 200}   # splats staged per batch by the forward instantiation that serves K
BWD_BATCH = {0: 208, 16: 224, 26: 224, 27: 224, 5: 208}   # ... by the backward's; the geometry-only backward: 208
GEO_BATCH = 208
W2, H2 = 32, 16                                            # two tiles


# ---- scenes: lists of (u, v, z, sigma_x, sigma_y, opacity), see test_gpu_fwd_visit_loop._scene ----
def exact_list(n, seed=21):
    """n splats of sigma 100 px centred above and to the right of the two tiles: every one of them is on both tiles' lists and contributes
    to every pixel (alpha 0.0050-0.0058, well above 1/255; T stays above 0.04 at n = 481), so both lists hold exactly n entries and every
    pixel's n_contrib is n: the backward walks exactly n entries too.  Entry 100 has alpha 0.25-0.29 and takes T from 0.58 to 0.43 at
    most on every pixel: the median crossing is nowhere a close call (as in test_gpu_fwd_visit_loop._crossing).  The centres lie
    beside the image in x as well as in y so that every pixel's contribution to a splat's dL_dmean2D has the same sign in both
    components: a centre above the middle of the image makes the x component a difference of two halves, of which fp32 sums over 448
    entries keep fewer digits than the comparison's 1e-4 asks of an entry that small."""
    r = np.random.RandomState(seed)
    z = _depths(max(n, 1), r)
    return [(48.0 + r.uniform(-1, 1), -20.0 + r.uniform(-1, 1), z[i], 100.0, 100.0, 0.3 if i == 100 else 0.006) for i in range(n)]


def early_stop(front_at, n_front=40, n_behind=460, seed=9):
    """tile 0: `front_at` faint splats, then an opaque front over its left half (the pixels of two waves finish inside it), then faint
    ones behind over the whole tile, which the other two waves blend to the end.  front_at = 0: the front is in batch 1 and the left
    waves skip every later batch; front_at = 250: it is in batch 2 of the forward, and the backward's left waves skip its FIRST batch.
    Tile 1 holds a handful of entries."""
    r = np.random.RandomState(6)
    near = _many(front_at, seed + 1, 0.012, z0=0.5, u_range=(0.0, 16.0)) if front_at else []
    near = [(u, v, 0.5 + 0.4 * i / max(front_at, 1), sx, sy, op) for i, (u, v, z, sx, sy, op) in enumerate(near)]
    front = [(r.uniform(1.0, 5.0), 8.0, 1.0 + 0.01 * i, 2.5, 8.0, 0.99) for i in range(n_front)]
    other = [(24.0 + r.uniform(-3, 3), 8.0 + r.uniform(-3, 3), 3.0 + 0.1 * i, 1.0, 1.0, 0.3) for i in range(5)]
    return near + front + _many(n_behind, seed, 0.012) + other


QUAD_CENTRE = [(4.0, 4.0), (12.0, 4.0), (4.0, 12.0), (12.0, 12.0)]


def empty_middle(n=720, gap=(225, 505), seed=14):
    """one tile (the second stays empty), n small splats (sigma 0.4 px: alpha reaches 1/255 within 2.2 px) dealt round the centres of the
    four 8x8 quadrants in depth order — except that between list positions gap[0] and gap[1] none goes to quadrant 0.  The forward's second
    batch (240..479) and the backward's second (about 272..495, counted from the last contributor) lie inside the gap: the wave of quadrant
    0 has an empty list there, between two batches in which it has work."""
    r = np.random.RandomState(seed)
    z = _depths(n, r)
    out = []
    for i in range(n):
        q = i % 4
        if q == 0 and gap[0] <= i < gap[1]:
            q = 1 + (i // 4) % 3
        cx, cy = QUAD_CENTRE[q]
        out.append((cx + r.uniform(-1.2, 1.2), cy + r.uniform(-1.2, 1.2), z[i], 0.4, 0.4, 0.02))
    return out


def with_culled(splats):
    """every fifth Gaussian behind the camera: culled, radius 0, on no list; the lists' ids are no longer consecutive"""
    out = []
    for i, s in enumerate(splats):
        out.append(s)
        if i % 4 == 3:
            out.append((s[0], s[1], -1.0, s[3], s[4], s[5]))
    return out


# ---- one oracle run per scene, shared by the tests that need it ----
_ORACLE = {}


def _oracle(key, W, H, K, splats, semantic=True):
    if key not in _ORACLE:
        cam, sc = _scene(W, H, K, splats)
        up = _upstream(W, H, K)
        out_o, gr_o, st_o = run_oracle(cam, sc, up, semantic=semantic)
        assert st_o.bounds_info["overflow_pixels"] == 0, st_o.bounds_info
        assert int(np.asarray(st_o.field("tie_pixels")).sum()) == 0, "the scene has tie-risk pixels: change its seed"
        st = {n: np.asarray(st_o.field(n)).copy() for n in ("n_contrib", "median_pos", "final_T", "vals", "ranges")}
        allow = {n: tie_allowance(n, st_o, out_o[n].shape, "pixel") for n in out_o if n in ("color", "depth", "opacity", "semantic", "mask")}
        allow["final_T"] = tie_allowance("opacity", st_o, (W * H,), "pixel")
        gallow = {n: tie_allowance("grad " + n, st_o, gr_o[n].shape, "gauss") for n in gr_o}
        st_o.free()
        _ORACLE[key] = (cam, sc, up, out_o, gr_o, st, allow, gallow)
    return _ORACLE[key]


def _check(key, W, H, K, splats, semantic=True):
    """forward and full backward on the GPU against the oracle; returns the oracle's per-pixel state"""
    cam, sc, up, out_o, gr_o, st, allow, gallow = _oracle(key, W, H, K, splats, semantic)
    out_g, gr_g, st_g = run_gpu(cam, sc, up, semantic=semantic, want_state=True)
    assert np.array_equal(out_g["radii"], out_o["radii"]), "radii"
    assert st_g["num_rendered"] == out_o["num_rendered"], "num_rendered"
    assert np.array_equal(st_g["vals"], st["vals"]), "sorted lists"
    assert np.array_equal(st_g["ranges"], st["ranges"]), "tile ranges"
    for n in ("n_contrib", "median_pos"):
        got, exp = st_g[n].reshape(-1), st[n].reshape(-1).astype(np.uint32)
        bad = got != exp
        assert not bad.any(), "%s differs on %d pixels, first at %d: %d vs %d" % (n, int(bad.sum()), int(np.argmax(bad)), int(got[np.argmax(bad)]),
                                                                                    int(exp[np.argmax(bad)]))
    assert_close("final_T", st_g["final_T"], st["final_T"].reshape(-1), allowance=allow["final_T"])
    for n in ("color", "depth", "opacity") + (("semantic",) if semantic else ("mask",)):
        assert_close(n, out_g[n], out_o[n], allowance=allow[n])
    assert_close("median_depth", out_g["median_depth"], out_o["median_depth"])
    for n in gr_o:
        assert_close("grad " + n, gr_g[n], gr_o[n], allowance=gallow[n])
    return {n: st[n].reshape(H, W) for n in ("n_contrib", "median_pos", "final_T")}


def _check_geometry_only(key, W, H, K, splats):
    """only means3D / means2D ask for a gradient: the geometry-only variant of the backward tile kernel, against the same oracle run"""
    from diff_gaussian_rasterization import GaussianRasterizer_semantic
    from harness import _cam_to
    cam, sc, up, out_o, gr_o, st, allow, gallow = _oracle(key, W, H, K, splats)
    dev = torch.device("cuda:0")
    P = sc["means3D"].shape[0]
    means3D = sc["means3D"].to(dev).clone().requires_grad_(True)
    means2D = torch.zeros(P, 3, device=dev, requires_grad=True)
    rest = {n: sc[n].to(dev).clone() for n in ("opacities", "colors_precomp", "scales", "rotations", "semantics_precomp")}
    color, radii, sem, depth, median, opacity = GaussianRasterizer_semantic(_cam_to(cam, dev))(means3D=means3D, means2D=means2D, **rest)
    loss = (sem * up["semantic"].to(dev)).sum() + (color * up["color"].to(dev)).sum() + (depth * up["depth"].to(dev)).sum() \
        + (median * up["median"].to(dev)).sum() + (opacity * up["opacity"].to(dev)).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert np.array_equal(radii.cpu().numpy(), out_o["radii"]), "radii"
    assert_close("grad means3D (geometry-only)", means3D.grad.cpu().numpy(), gr_o["means3D"], allowance=gallow["means3D"])
    assert_close("grad means2D (geometry-only)", means2D.grad.cpu().numpy(), gr_o["means2D"], allowance=gallow["means2D"])


# ---- list lengths ----
LENGTHS = [0, 1, 239, 240, 241, 480, 481, 223, 224, 225, 448, 449]


@pytest.mark.parametrize("n", LENGTHS)
def test_list_length(n):
    """K = 26: lists of exactly n entries on both tiles, every pixel blends all n"""
    st = _check(("exact", 26, n), W2, H2, 26, exact_list(n) if n else [(16.0, 8.0, -1.0, 1.0, 1.0, 0.5)])   # n = 0: one culled Gaussian
    assert (st["n_contrib"] == n).all()
    if n >= 240:
        assert st["median_pos"].min() > 0 and st["final_T"].max() < 0.5


# ---- kernel variants: a list one entry longer than the forward's batch, and one entry longer than two of the backward's ----
@pytest.mark.parametrize("K", [0, 16, 27, 5])
@pytest.mark.parametrize("which", ["fwd_batch_plus_1", "two_bwd_batches_plus_1"])
def test_kernel_variants(which, K):
    n = FWD_BATCH[K] + 1 if which == "fwd_batch_plus_1" else 2 * BWD_BATCH[K] + 1
    st = _check(("exact", K, n), W2, H2, K, exact_list(n))
    assert (st["n_contrib"] == n).all()


@pytest.mark.parametrize("n", [241, 417])
def test_non_semantic_render(n):
    st = _check(("exact-mask", 0, n), W2, H2, 0, exact_list(n), semantic=False)
    assert (st["n_contrib"] == n).all()


@pytest.mark.parametrize("n", [1, GEO_BATCH - 1, GEO_BATCH, GEO_BATCH + 1, 2 * GEO_BATCH + 1, 481])
def test_geometry_only_backward(n):
    _check_geometry_only(("exact", 26, n), W2, H2, 26, exact_list(n))


# ---- early stop, empty wave list ----
@pytest.mark.parametrize("front_at", [0, 250])
@pytest.mark.parametrize("K", [26, 0])
def test_two_waves_stop_early(K, front_at):
    key = ("early", K, front_at)
    st = _check(key, W2, H2, K, early_stop(front_at))
    n, fT = st["n_contrib"], st["final_T"]
    hi = int(n[:, :16].max())
    assert (fT[:, :8] < 0.01).all() and n[:, :8].max() <= front_at + 40                # the left half stops inside the front
    assert hi > front_at + 40 + 2 * 240 - 60 and n[:8, 8:16].max() > hi - 60 and n[8:, 8:16].max() > hi - 60   # the right half goes on
    if front_at:
        assert n[:, :8].max() > 240 and hi - 224 >= n[:, :8].max()                     # front in batch 2; the backward's first batch is skipped
    if K == 26:
        _check_geometry_only(key, W2, H2, K, early_stop(front_at))


@pytest.mark.parametrize("K", [26, 16])
def test_wave_with_an_empty_list_in_the_middle_batch(K):
    key = ("empty-middle", K)
    st = _check(key, W2, H2, K, empty_middle())
    n = st["n_contrib"]
    hi = int(n.max())
    q0 = n[:8, :8]
    assert hi > 700 and q0.max() > 505                                               # quadrant 0 has work behind the gap ...
    assert not ((q0 > 225) & (q0 <= 505)).any()                                      # ... and none inside it
    assert hi - 224 <= 505 and hi - 448 >= 225                                       # the backward's second batch lies inside the gap
    assert (n[:8, 8:16] > 240).any() and (n[8:, :8] > 240).any()
    if K == 26:
        _check_geometry_only(key, W2, H2, K, empty_middle())


# ---- culled Gaussians ----
@pytest.mark.parametrize("n", [241, 449])
def test_every_fifth_gaussian_culled(n):
    splats = with_culled(exact_list(n))
    st = _check(("culled", 26, n), W2, H2, 26, splats)
    assert (st["n_contrib"] == n).all() and len(splats) == n + n // 4
    _check_geometry_only(("culled", 26, n), W2, H2, 26, splats)


# ---- the forward's two launch paths ----
def test_forward_launch_paths(monkeypatch):
    """the speculative launch (list bases resolved on the device from num_rendered: the binning buffer is roomy) and the fall-back
    (buffer too small: the call grows it and launches again with host-resolved bases), on a list of three batches"""
    from diff_gaussian_rasterization import _C
    if os.environ.get("HSR_ASYNC_FORWARD"):
        pytest.skip("the blocking forward's grow-and-rerun fall-back is not taken when the non-blocking forward is forced on")
    n = 481
    splats = exact_list(n)
    key = (torch.device("cuda:0").index, n, W2, H2)
    _C._binning_hint.pop(key, None)
    _check(("exact", 26, n), W2, H2, 26, splats)                  # default hint 4 P >= 2 P entries: speculative
    R = _C._binning_hint[key]
    assert R == 2 * n
    monkeypatch.setitem(_C._binning_hint, key, 1)                 # far too small: fall-back
    _check(("exact", 26, n), W2, H2, 26, splats)
    assert _C._binning_hint[key] == R
