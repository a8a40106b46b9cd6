"""-m gpu: the forward tile kernel's STAGED visit loop (hsr_render_fwd.hip, the per-lane kernels: K = 0, 16, 26, the 32-channel chunk and
the non-semantic variant) against the CPU oracle.

The loop is software-pipelined by hand: while trip k blends, the record of trip k + 1 has been requested and its alpha is being computed,
and the list byte of trip k + 2 is in flight; a prologue does trip 0's share in front of the loop; nothing staged survives a batch.  The
scenes are hand-placed on one to three 16x16 tiles with the conventions of test_gpu_fwd_visit_loop.py (whose small scene builder is
copied here), and each is aimed at something the rotation alone can break:

  1. wave trip counts m = 1, 2, 3 (the prologue with nothing, one and two real trips behind it; the other waves run it with m = 0);
  2. a sub-block whose list holds every entry of a full batch (the look-ahead reads index m + 1 of a full list), and one entry more
     (the second batch has m = 1);
  3. strong entries (opacity 0.3) and entries below 1/255 (0.0025) in turn on one sub-block: the middle pixels finish half-way down the
     list and see every later entry with T = 0 while their neighbours go on (an entry below 1/255 is on the tile's list and on no
     sub-block's, so the staged slots skip over it);
  4. a pixel that finishes on trip k while the entry of trip k + 1, whose alpha was computed before the pixel finished, is an opaque one:
     once inside a batch, once with k the last trip of a batch; nothing of trip k + 1 may reach the pixel;
  5. the last trip of batch 1 and the first of batch 2 both contributing, with different splats, on a group whose neighbour groups in
     the wave are empty in batch 2;
  6. the median crossing and the last contributor on trip 0 of a batch and on its trip m - 1;
  7. a partial tile (image 24x20) under the list of 3.

Every scene is built so that the oracle flags no tie-risk pixel (asserted; the seeds were picked on the CPU), so n_contrib and median_pos
are compared exactly on every pixel.  Tolerances for the images and gradients: harness.assert_close (1e-4, tensor-wide and element-wise)
plus the oracle's tie bound (zero here).  What each scene was built to do is asserted on the oracle's state (expectations)."""
import numpy as np
import pytest
import torch

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


def _narrow(u, v, z, r, opacity, jitter=0.15):
    """sigma 0.4 px: alpha reaches 1/255 within 2.2 px of the centre at most, so a splat at the middle of a 4x4 sub-block is on that
    sub-block's list and on no other"""
    return (u + r.uniform(-jitter, jitter), v + r.uniform(-jitter, jitter), z, 0.4, 0.4, opacity)


def _wide(z, r, opacity, sigma=100.0):
    """centred 20 px above a 16x16 image so that no pixel sits on a centre: alpha is nearly the opacity on the whole tile (within 5 % at
    sigma 100, within 0.4 % at sigma 400) and every sub-block lists the entry if its opacity is above 1/255"""
    return (8.0 + r.uniform(-1, 1), -20.0 + r.uniform(-1, 1), z, sigma, sigma, opacity)


# ---- the scenes: name -> (W, H, splats(K)) ----
def trips(K, counts, seed=21):
    """wave 0 of the one tile: counts[g] narrow splats of opacity 0.3 on sub-block g (pixel block 4 (g & 1), 4 (g >> 1)), depths interleaved"""
    r = np.random.RandomState(seed)
    where = [g for g, c in enumerate(counts) for _ in range(c)]
    r.shuffle(where)
    z = _depths(len(where), r)
    return [_narrow(2.0 + 4.0 * (g & 1), 2.0 + 4.0 * (g >> 1), z[i], r, 0.3) for i, g in enumerate(where)]


def full_batch(K, extra, seed=22):
    """BATCH + extra faint splats (sigma 2 .. 3.5 px) whose centres lie inside sub-block 3 of wave 0 (pixels 4..7 x 4..7): its list holds
    every entry of the batch"""
    r = np.random.RandomState(seed)
    n = BATCH[K] + extra
    z = _depths(n, r)
    return [(r.uniform(4.5, 7.5), r.uniform(4.5, 7.5), z[i], r.uniform(2.0, 3.5), r.uniform(2.0, 3.5), 0.012) for i in range(n)]


def alternating(K, u=6.0, v=6.0, n=160, seed=23):
    """opacities 0.3 and 0.0025 in turn, all narrow and on one sub-block; its middle pixels (alpha 0.2) finish after some forty strong
    entries, the outer ones (alpha 0.02) go on to the end"""
    r = np.random.RandomState(seed)
    z = _depths(n, r)
    return [_narrow(u, v, z[i], r, 0.3 if i % 2 == 0 else 0.0025) for i in range(n)]


def finish_then_strong(K, first, n_after=12, seed=26):
    """`first` wide faint entries (alpha 0.0052: T falls to 0.29 .. 0.39), then four opaque ones (sigma 400 px: alpha 0.986 .. 0.989 on
    every pixel), then faint ones.  The first opaque entry leaves T near 4e-3, the second takes it to 3.6e-5 .. 7.7e-5 < 1e-4 on every
    pixel: the pixel finishes there, on list entry first + 1, and the third opaque entry — whose alpha the staged loop has computed by
    then — must not reach it."""
    r = np.random.RandomState(seed)
    n = first + 4 + n_after
    z = _depths(n, r)
    return [_wide(z[i], r, 0.0052) if (i < first or i >= first + 4) else _wide(z[i], r, 0.99, sigma=400.0) for i in range(n)]


def batch_seam(K, seed=25):
    """narrow splats of opacity 0.05 on the four sub-blocks of wave 0 in turn through the first batch, whose last entry is on sub-block 0;
    the three entries of the second batch are all on sub-block 0: its neighbours' lists are empty there"""
    r = np.random.RandomState(seed)
    B = BATCH[K]
    z = _depths(B + 3, r)
    out = []
    for i in range(B + 3):
        g = 0 if i >= B - 1 else i % 4
        out.append(_narrow(2.0 + 4.0 * (g & 1), 2.0 + 4.0 * (g >> 1), z[i], r, 0.05))
    return out


def crossing(K, med, last, n, seed=13):
    """one tile under n wide splats.  Before `med`: a hundred of alpha 0.0052 (T falls to 0.6), the rest at opacity 0.0025 < 1/255 (tile
    list entries that are on no sub-block's list); entry `med` has alpha 0.3 and takes T through 0.5 on every pixel; between `med` and
    `last` every fourth entry contributes faintly; entry `last` (>= med) is the last one above 1/255."""
    r = np.random.RandomState(seed)
    z = _depths(n, r)
    contributing = set(np.linspace(0, med - 1, 100).astype(int).tolist()) | set(range(med + 2, last, 4))
    out = []
    for i in range(n):
        op = 0.3 if i == med else (0.2 if i == last else (0.0052 if i in contributing else 0.0025))
        out.append(_wide(z[i], r, op))
    return out


def _scenes_for(K):
    B = BATCH[K]
    return {
        "trips_1": (16, 16, trips(K, (1, 0, 0, 0))),
        "trips_2": (16, 16, trips(K, (2, 0, 0, 0))),
        "trips_3_and_2": (16, 16, trips(K, (3, 2, 0, 0))),
        "full_batch": (16, 16, full_batch(K, 0)),
        "full_batch_and_one": (16, 16, full_batch(K, 1)),
        "alternating": (16, 16, alternating(K)),
        "finish_inside_batch": (16, 16, finish_then_strong(K, 180)),
        "finish_on_last_of_batch": (16, 16, finish_then_strong(K, B - 2)),
        "batch_seam": (16, 16, batch_seam(K)),
        "cross_and_last_on_trip_0": (16, 16, crossing(K, B, B, B + 40)),
        "cross_on_trip_0_last_on_trip_m1": (16, 16, crossing(K, B, B + 39, B + 40)),
        "cross_and_last_on_trip_m1": (16, 16, crossing(K, B - 1, B - 1, B + 40)),
        "cross_on_trip_m1_last_on_trip_0": (16, 16, crossing(K, B - 1, B, B + 40)),
        "partial_tile": (24, 20, alternating(K, u=22.0, v=18.0)),
    }


SCENE_NAMES = list(_scenes_for(26))


def oracle_of(cam, sc, up, semantic=True):
    """the oracle's outputs, gradients and state for a scene, with the assertion that none of its pixels is a tie risk"""
    out_o, gr_o, st_o = run_oracle(cam, sc, up, semantic=semantic)
    assert st_o.bounds_info["overflow_pixels"] == 0, st_o.bounds_info
    assert int(np.asarray(st_o.field("tie_pixels")).sum()) == 0, "the scene has tie-risk pixels: change its seed"
    return out_o, gr_o, st_o


def oracle_state(st_o, W, H):
    return {n: np.asarray(st_o.field(n)).reshape(-1).copy().reshape(H, W) for n in ("n_contrib", "median_pos", "final_T")}


def _check(cam, sc, up, semantic=True):
    out_o, gr_o, st_o = oracle_of(cam, sc, up, semantic)
    try:
        out_g, gr_g, st_g = run_gpu(cam, sc, up, semantic=semantic, want_state=True)
        H, W = cam["image_height"], cam["image_width"]
        exp = oracle_state(st_o, W, H)
        for n in ("n_contrib", "median_pos"):
            e = exp[n].reshape(-1)
            bad = st_g[n].reshape(-1) != e.astype(np.uint32)
            assert not bad.any(), "%s differs on %d pixels, first at %d: %d vs %d" % (
                n, int(bad.sum()), int(np.argmax(bad)), int(st_g[n].reshape(-1)[np.argmax(bad)]), int(e[np.argmax(bad)]))
        assert_close("final_T", st_g["final_T"], exp["final_T"].reshape(-1), allowance=tie_allowance("opacity", st_o, (W * H,), "pixel"))
        for n in ("color", "depth", "opacity") + (("semantic",) if semantic else ("mask",)):
            assert_close(n, out_g[n], out_o[n], allowance=tie_allowance(n, st_o, out_g[n].shape, "pixel"))
        assert_close("median_depth", out_g["median_depth"], out_o["median_depth"])
        for n in gr_o:   # the backward reads the masks the forward left
            assert_close("grad " + n, gr_g[n], gr_o[n], allowance=tie_allowance("grad " + n, st_o, gr_g[n].shape, "gauss"))
        return exp
    finally:
        st_o.free()


def expectations(name, K, st):
    """what the scene was built to do, asserted on the ORACLE's state (so it can be checked without a GPU)"""
    n, med, fT = st["n_contrib"], st["median_pos"], st["final_T"]
    B = BATCH[K]
    if name.startswith("trips"):
        counts = {"trips_1": (1, 0), "trips_2": (2, 0), "trips_3_and_2": (3, 2)}[name]
        total = sum(counts)
        # every entry is the last contributor of some pixel of ITS sub-block, and no other pixel sees anything
        seen0, seen1 = set(n[:4, :4].reshape(-1).tolist()) - {0}, set(n[:4, 4:8].reshape(-1).tolist()) - {0}
        assert len(seen0 | seen1) >= 1 and max(seen0 | seen1) == total and not (seen0 & seen1)
        assert n[1:3, 1:3].max() >= counts[0] and (counts[1] == 0) == (len(seen1) == 0)
        rest = n.copy()
        rest[:4, :8] = 0
        assert rest.max() == 0
    elif name == "full_batch":
        assert n[4:8, 4:8].max() == B and (fT > 1e-3).all()
    elif name == "full_batch_and_one":
        assert n[4:8, 4:8].max() == B + 1 and (fT > 1e-3).all()
    elif name in ("alternating", "partial_tile"):
        y0, x0 = (4, 4) if name == "alternating" else (16, 20)
        blk, blkT = n[y0:y0 + 4, x0:x0 + 4], fT[y0:y0 + 4, x0:x0 + 4]
        assert (blk[blk > 0] % 2 == 1).all()                        # only the strong entries (even list positions) ever contribute
        assert blk[1:3, 1:3].max() < 159 and (blkT[1:3, 1:3] < 1e-3).all()   # the middle finishes early ...
        assert blk.max() == 159                                     # ... while the outer pixels go on to the last strong entry
        rest = n.copy()
        rest[y0:y0 + 4, x0:x0 + 4] = 0
        assert rest.max() == 0
    elif name.startswith("finish"):
        first = 180 if name == "finish_inside_batch" else B - 2
        assert (n == first + 1).all() and (fT < 1e-2).all() and (fT > 1e-4).all()   # finished on entry first + 1: the last contributor is `first`
    elif name == "batch_seam":
        assert n[:4, :4].max() == B + 3   # (which entries besides the last one reached a pixel is for the images to say)
        assert 0 < n[:4, 4:8].max() < B and 0 < n[4:8, :4].max() < B and 0 < n[4:8, 4:8].max() < B
        assert n[8:, :].max() == 0 and n[:, 8:].max() == 0
    elif name.startswith("cross"):
        m, last = {"cross_and_last_on_trip_0": (B, B), "cross_on_trip_0_last_on_trip_m1": (B, B + 39),
                   "cross_and_last_on_trip_m1": (B - 1, B - 1), "cross_on_trip_m1_last_on_trip_0": (B - 1, B)}[name]
        assert (med == m + 1).all() and (n == last + 1).all()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_visit_stages(name, K):
    W, H, splats = _scenes_for(K)[name]
    cam, sc = _scene(W, H, K, splats)
    expectations(name, K, _check(cam, sc, _upstream(W, H, K)))


@pytest.mark.parametrize("name", ["trips_3_and_2", "full_batch_and_one", "alternating", "finish_on_last_of_batch", "batch_seam",
                                  "cross_on_trip_0_last_on_trip_m1", "partial_tile"])
def test_non_semantic_render(name):
    W, H, splats = _scenes_for(0)[name]
    cam, sc = _scene(W, H, 0, splats)
    expectations(name, 0, _check(cam, sc, _upstream(W, H, 0), semantic=False))
