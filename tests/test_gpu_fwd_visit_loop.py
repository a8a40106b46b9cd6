"""-m gpu: the forward tile kernel's visit loop (hsr_render_fwd.hip, the per-lane kernels: K = 0, 16, 26, the 32-channel chunk and the
non-semantic variant) against the CPU oracle.

The loop has no validity predicate: a 16-lane group whose list is shorter than the wave's iteration count visits a dummy entry of opacity 0,
and a finished pixel is a pixel whose running transmittance is 0.  The scenes are hand-placed on one to three 16x16 tiles so that each of
these is exercised on purpose: a tile with no entry, with one entry, with entries in one sub-block only (fifteen groups on dummies); groups
of one wave with lists of very different lengths, one of them empty in the second batch; lists of two and three batches with the median
crossing and the last contributor on the last entry of a batch and on the first of the next; pixels, and whole waves, that finish early
while their neighbours go on; pixels that finish as early as the blend allows; partial tiles.

Every scene is built so that the oracle flags no tie-risk pixel (asserted), so n_contrib and median_pos are compared exactly on every pixel.
Tolerances for the images and gradients: harness.assert_close (1e-4, tensor-wide and element-wise) plus the oracle's tie bound (zero here)."""
import numpy as np
import pytest
import torch

import scenes
from harness import assert_close, run_gpu, run_oracle, tie_allowance
from hsr_utils.camera import replica_intrinsics, setup_camera_tensors
from hsr_utils.synthetic import make_upstream_grads

pytestmark = pytest.mark.gpu

KS = [0, 16, 26, 5]                          # 5: rendered by the 32-channel instantiation
BATCH = {0: 240, 16: 240, 26: 240, 5: 200}   # splats staged per batch by the instantiation that serves K


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


def _upstream(W, H, K):
    return {n: v * float(W * H) for n, v in make_upstream_grads(W, H, K, seed=1).items()}   # O(1) per pixel: errors read as relative


def _depths(n, r, z0=2.0, span=4.0):
    return [z0 + span * (i + r.uniform(0.2, 0.8)) / n for i in range(n)]


def _many(n, seed, opacity, z0=2.0, u_range=(0.0, 16.0), v_range=(0.0, 16.0), sigma=(2.0, 3.5)):
    r = np.random.RandomState(seed)
    z = _depths(n, r, z0)
    return [(r.uniform(*u_range), r.uniform(*v_range), z[i], r.uniform(*sigma), r.uniform(*sigma), opacity) for i in range(n)]


# ---- the scenes: name -> (W, H, splats(K)) ----
def sparse_tiles(K):
    """48x16, three tiles: no entry / one entry / five entries, all inside sub-block (1, 1) of their tile (sigma 0.4 px: alpha reaches
    1/255 within 2.2 px of the centre and the 3-sigma rectangle stays inside the tile)"""
    r = np.random.RandomState(11)
    return [(22.0, 6.0, 2.0, 0.4, 0.4, 0.8)] + [(38.0 + r.uniform(-0.15, 0.15), 6.0 + r.uniform(-0.15, 0.15), 2.0 + 0.5 * i, 0.4, 0.4, 0.3)
                                                for i in range(5)]


def uneven_groups(K):
    """one tile, wave 0 only: sub-block 1 has ~300 faint entries through all depths, sub-block 0 thirty among the nearest (first batch
    only: its list is empty in the second), sub-block 2 three, sub-block 3 none; the other three waves have nothing at all"""
    r = np.random.RandomState(12)
    n = 300
    z = _depths(n + 33, r)
    out = []
    near = set(range(5, 65, 2))        # 30 of the first 65 depths go to sub-block 0
    few = {20, 150, 310}
    for i in range(n + 33):
        if i in few:
            out.append((2.0 + r.uniform(-0.4, 0.4), 6.0 + r.uniform(-0.4, 0.4), z[i], 0.4, 0.4, 0.3))
        elif i in near:
            out.append((2.0 + r.uniform(-0.4, 0.4), 2.0 + r.uniform(-0.4, 0.4), z[i], 0.4, 0.4, 0.05))
        else:
            out.append((6.0 + r.uniform(-0.4, 0.4), 2.0 + r.uniform(-0.4, 0.4), z[i], 0.4, 0.4, 0.012))
    return out


def two_batches(K):
    return _many(BATCH[K] + 1, 5, 0.012)


def three_batches(K):
    return _many(600, 5, 0.012)


def _crossing(K, med, last, n=300):
    """one tile under n wide splats (sigma 100 px, centred 20 px above the image so that no pixel sits on a centre: alpha varies by 5 %
    over the tile).  Entries before `med`: a hundred of alpha 0.0052
    (T falls to 0.6), the rest at opacity 0.0025 < 1/255 (list entries that never contribute); entry `med` has alpha 0.3 and takes T
    through 0.5 on every pixel; entry `last` (>= med) is the last one above 1/255."""
    r = np.random.RandomState(13)
    z = _depths(n, r)
    contributing = set(np.linspace(0, med - 1, 100).astype(int).tolist())
    out = []
    for i in range(n):
        op = 0.3 if i == med else (0.2 if i == last else (0.0052 if (i < med and i in contributing) else 0.0025))
        out.append((8.0 + r.uniform(-1, 1), -20.0 + r.uniform(-1, 1), z[i], 100.0, 100.0, op))
    return out


def early_finish(K):
    """40 opaque splats in front over the left half only (tall, 2.5 px wide, centred on columns 1..5), 460 faint ones behind them"""
    r = np.random.RandomState(6)
    front = [(r.uniform(1.0, 5.0), 8.0, 1.0 + 0.01 * i, 2.5, 8.0, 0.99) for i in range(40)]
    return front + _many(460, 9, 0.012)   # seed 7 puts a decision of one pixel within 2e-6 of its threshold


def earliest_finish(K):
    """the same splat of opacity 0.99 three times over the same pixels, faint ones behind.  alpha <= 0.99 and T starts at 1, so no pixel
    can finish on its first entry, and one that finishes on its second does so with T (1 - 0.99)^2 within 2e-6 of the 1e-4 threshold (a
    tie by the oracle's measure): the centre sits between pixel centres (alpha 0.986 at most), the second visit leaves T ~ 1.9e-4 and
    the third finishes the pixels near the centre; the pixels further out finish later or not at all."""
    return [(8.0, 8.0, 1.0 + 0.01 * i, 8.0, 8.0, 0.99) for i in range(3)] + _many(60, 8, 0.012)


def _scenes_for(K):
    B = BATCH[K]
    return {
        "sparse_tiles": (48, 16, sparse_tiles(K)),
        "uneven_groups": (16, 16, uneven_groups(K)),
        "two_batches": (16, 16, two_batches(K)),
        "three_batches": (16, 16, three_batches(K)),
        "cross_last_of_batch": (16, 16, _crossing(K, B - 1, B - 1)),
        "cross_first_of_next": (16, 16, _crossing(K, B, B)),
        "cross_then_last_over_the_boundary": (16, 16, _crossing(K, B - 1, B)),
        "early_finish": (16, 16, early_finish(K)),
        "earliest_finish": (16, 16, earliest_finish(K)),
    }


SCENE_NAMES = list(_scenes_for(26))


def oracle_of(cam, sc, up, semantic=True):
    """the oracle's outputs, gradients and state for a scene, with the assertion that none of its pixels is a tie risk"""
    out_o, gr_o, st_o = run_oracle(cam, sc, up, semantic=semantic)
    assert st_o.bounds_info["overflow_pixels"] == 0, st_o.bounds_info
    assert int(np.asarray(st_o.field("tie_pixels")).sum()) == 0, "the scene has tie-risk pixels: change its seed"
    return out_o, gr_o, st_o


def _check(cam, sc, up, semantic=True):
    out_o, gr_o, st_o = oracle_of(cam, sc, up, semantic)
    try:
        out_g, gr_g, st_g = run_gpu(cam, sc, up, semantic=semantic, want_state=True)
        H, W = cam["image_height"], cam["image_width"]
        exp = {n: np.asarray(st_o.field(n)).reshape(-1).copy() for n in ("n_contrib", "median_pos", "final_T")}
        for n in ("n_contrib", "median_pos"):
            bad = st_g[n].reshape(-1) != exp[n].astype(np.uint32)
            assert not bad.any(), "%s differs on %d pixels, first at %d: %d vs %d" % (
                n, int(bad.sum()), int(np.argmax(bad)), int(st_g[n].reshape(-1)[np.argmax(bad)]), int(exp[n][np.argmax(bad)]))
        assert_close("final_T", st_g["final_T"], exp["final_T"], allowance=tie_allowance("opacity", st_o, (W * H,), "pixel"))
        for n in ("color", "depth", "opacity") + (("semantic",) if semantic else ("mask",)):
            assert_close(n, out_g[n], out_o[n], allowance=tie_allowance(n, st_o, out_g[n].shape, "pixel"))
        assert_close("median_depth", out_g["median_depth"], out_o["median_depth"])
        for n in gr_o:   # the backward reads the masks the forward left
            assert_close("grad " + n, gr_g[n], gr_o[n], allowance=tie_allowance("grad " + n, st_o, gr_g[n].shape, "gauss"))
        return {n: v.reshape(H, W) for n, v in exp.items()}, out_o
    finally:
        st_o.free()


def expectations(name, K, st):
    """what the scene was built to do, asserted on the ORACLE's state (so it can be checked without a GPU)"""
    n, med, fT = st["n_contrib"], st["median_pos"], st["final_T"]
    B = BATCH[K]
    if name == "sparse_tiles":
        assert n[:, :16].max() == 0 and (fT[:, :16] == 1.0).all()                    # the tile with no entry
        inside = np.zeros_like(n, bool)
        inside[4:8, 20:24] = True
        inside[4:8, 36:40] = True
        assert n[~inside].max() == 0 and n[4:8, 20:24].min() == 1 and n[4:8, 36:40].max() == 5
    elif name == "uneven_groups":
        assert n[:4, 4:8].max() > B + 60 and 0 < n[:4, :4].max() <= 65 and n[4:8, :4].max() > B
        assert n[4:8, 4:8].max() == 0 and n[8:, :].max() == 0 and n[:, 8:].max() == 0
    elif name == "two_batches":
        assert n.max() == B + 1
    elif name == "three_batches":
        assert n.max() > 2 * B
    elif name.startswith("cross"):
        m, last = {"cross_last_of_batch": (B - 1, B - 1), "cross_first_of_next": (B, B), "cross_then_last_over_the_boundary": (B - 1, B)}[name]
        assert (med == m + 1).all() and (n == last + 1).all()
    elif name == "early_finish":
        hi = int(n.max())
        assert hi > 2 * B and n[:, :8].max() <= 40 and (fT[:, :8] < 0.01).all()      # the left half stops inside the opaque front
        assert n[:8, 8:].max() == hi or n[8:, 8:].max() == hi                        # the right half goes on to the end of the list
    elif name == "earliest_finish":
        assert (n[6:10, 6:10] == 2).all() and (fT[6:10, 6:10] < 0.01).all()          # finished by the third entry: two contributors
        assert n.max() > 3


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_visit_loop(name, K):
    W, H, splats = _scenes_for(K)[name]
    cam, sc = _scene(W, H, K, splats)
    st, _ = _check(cam, sc, _upstream(W, H, K))
    expectations(name, K, st)


@pytest.mark.parametrize("K", KS)
def test_partial_tiles(K):
    """40x24: lanes outside the image start finished and store nothing"""
    cam, sc, up = scenes.build(40, 24, 200, K, seed=5, kind="aniso", scale_mult=2.0)
    _check(cam, sc, up)


@pytest.mark.parametrize("name", ["uneven_groups", "three_batches", "early_finish"])
def test_non_semantic_render(name):
    W, H, splats = _scenes_for(0)[name]
    cam, sc = _scene(W, H, 0, splats)
    st, _ = _check(cam, sc, _upstream(W, H, 0), semantic=False)
    expectations(name, 0, st)
