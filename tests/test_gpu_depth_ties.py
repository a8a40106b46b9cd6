"""-m gpu: list order among EQUAL depths, on first-frame-style maps (tests/scenes.py sensor_grid; tests/test_depth_ties_cpu.py holds the
scenes to their regime and states the figures).

On the random scenes of the rest of the suite two splats of a tile almost never share a depth, so the index half of the per-tile sort's
composite key decides nothing there.  Here 93-99.9 % of the neighbours in the sorted lists have equal keys and the lists are still
compared bit for bit with the oracle's, which covers, in hsr_sort.hip:

  * the low 32 bits of (depth bits << 32) | index in the register networks of tile_sort_pair_kernel (<= 256: `small`, exactly 256:
    `one_tile_256`; 257-512 and 513-1024: `first_frame`, `duplicates`, `wide`) and of block_sort_tile (1025-2048: `wide`, `deep`);
  * the Gaussian-index passes of ts_block_radix (`deep`: two of six passes; `deep_65537`: three of seven) and, with an odd number of
    passes, the copy of the segment back into the sorted pair at its end (P > 65 536 and tiles beyond 2 048 entries: `deep_65537`,
    and `deep_65537_two_exponents`, whose tiles hold depths on both sides of 2.0 — with depths of 2-4 m alone the last pass moves
    nothing and a build WITHOUT the copy still leaves the right lists behind);
  * both launch shapes of the per-tile sort (test_big_tiles_after_a_shallow_frame) and the emission-order path of HSR_SORT_IMPL=radix,
    whose block radix sort has no index passes and relies on the stability of every pass instead.

The *_shuffled cases number the Gaussians at random, so that ascending index is not raster order; `duplicates` appends copies of 1 000
Gaussians, as densification over existing points does."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scenes
from harness import run_gpu, run_oracle
from test_gpu_parity import _compare, _compare_integers

pytestmark = pytest.mark.gpu

MIN_TIE_SHARE = 0.9


def _run_case(name):
    """one TIE_CASES scene through the whole comparison (floats cases) or the bit-exact integer state alone"""
    import test_gpu_parity
    kw, lo_class, hi_class, floats = scenes.TIE_CASES[name]
    cam, sc, up = scenes.sensor_grid(**kw)
    if floats:
        before = len(test_gpu_parity.TIE_BOUNDED)
        _compare(cam, sc, up, True, "sr")
        print("%s: every list bit-equal to the oracle's; comparisons that needed the oracle's threshold-tie bound: %s"
              % (name, ", ".join(test_gpu_parity.TIE_BOUNDED[before:]) or "none"))
        return
    out_g, gr_g, st_g = run_gpu(cam, sc, up, semantic=True)
    out_o, gr_o, st_o = run_oracle(cam, sc, up, semantic=True)
    try:
        share = scenes.tie_share(st_g["keys"])
        print("%s: R %d, equal adjacent keys on the device %.4f; integer state only" % (name, st_g["num_rendered"], share))
        assert share >= MIN_TIE_SHARE
        _compare_integers(out_g, st_g, out_o, st_o)
    finally:
        st_o.free()


@pytest.mark.parametrize("name", list(scenes.TIE_CASES))
def test_parity_with_equal_depths(name):
    _run_case(name)


def test_the_sessions_own_first_frame_map():
    """The map hsr_utils.slam.initialize_first_timestep builds from a 96 x 64 frame whose depth image is quantised to millimetres, as the
    render variables of frame 0 (identity pose, every opacity sigmoid(0) = 0.5, isotropic scales): the product's map, not an imitation."""
    import oracle_lib as O
    from hsr_utils import slam, slam_helpers as SH
    from hsr_utils.camera import replica_intrinsics, setup_camera_tensors
    from hsr_utils.synthetic import make_upstream_grads
    W, H, levels = 96, 64, [2, 2]
    K = sum(levels)
    k = replica_intrinsics(W, H)
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    depth = scenes.sensor_grid_depth(xs.float(), ys.float(), H, 1.0).reshape(1, H, W)
    color = torch.rand(3, H, W, generator=torch.Generator(device="cpu").manual_seed(0))
    dev = torch.device("cuda:0")
    torch.manual_seed(7)    # the semantic rows are torch.rand on the device
    params, variables = slam.initialize_first_timestep(color.to(dev), depth.to(dev), torch.tensor(np.asarray(k), dtype=torch.float32).to(dev),
                                                       torch.eye(4, device=dev), 1, 3.0, "projective", "isotropic", num_semantic=levels)
    assert params["means3D"].shape[0] == W * H and params["semantic"].shape == (W * H, K)
    with torch.no_grad():
        rv = SH.transformed_params2rendervar_semantic(params, SH.transform_to_frame(params, 0, False, False))
        sc = {n: rv[n].detach().float().cpu().contiguous() for n in ("means3D", "colors_precomp", "rotations", "opacities", "scales",
                                                                    "semantics_precomp")}
    assert sc["scales"].shape == (W * H, 3) and bool((sc["opacities"] == 0.5).all())
    cam = setup_camera_tensors(W, H, k, np.eye(4))
    cam["bg"] = torch.zeros(3, dtype=torch.float32)
    up = {n: v * float(W * H) for n, v in make_upstream_grads(W, H, K, seed=1).items()}
    out, st = O.forward(cam, sc["means3D"], sc["opacities"], colors_precomp=sc["colors_precomp"], semantics_precomp=sc["semantics_precomp"],
                        scales=sc["scales"], rotations=sc["rotations"])
    share = scenes.tie_share(st.field("keys"))
    st.free()
    print("first-frame map of the session: P %d, R %d, equal adjacent keys %.4f" % (W * H, out["num_rendered"], share))
    assert share >= MIN_TIE_SHARE, share
    _compare(cam, sc, up, True, "sr")


def test_big_tiles_after_a_shallow_frame():
    """hsr_forward sizes the per-tile sort's launch from the entries per tile of the thread's PREVIOUS forward (g_last_per_tile,
    hsr_api.hip) whenever it enqueues the sort before it has read num_rendered back, i.e. whenever the binning buffer sized from the last
    count of this (device, P, W, H) has room.  In one process:
      1. `deep` with no hint for its size: 4 P entries of room do not hold its 22 758, so the call grows the buffer and sorts with the
         frame's own average (1 896 per tile > 800): the tiles beyond 1 024 entries get tile_sort_kernel, a launch of their own;
      2. `first_frame`: 495 entries per tile on average;
      3. `deep` again: the hint now fits, the sort is enqueued ahead with the previous frame's 495 <= 800, so tile_sort_pair_kernel sorts
         the 1 025-2 048 tiles and the block-radix tiles itself in its workgroup phase (big_too = 1), two tiles per workgroup.
    (With the opt-in non-blocking forward forced on for the whole run, step 3 is enqueued ahead in the same way with the hint of step 1.)"""
    from diff_gaussian_rasterization import _C
    deep, first = scenes.TIE_CASES["deep"][0], scenes.TIE_CASES["first_frame"][0]
    key = (torch.device("cuda:0").index or 0, (deep["W"] * deep["H"]), deep["W"], deep["H"])
    _C._binning_hint.pop(key, None)
    cam, sc, up = scenes.sensor_grid(**deep)
    _compare(cam, sc, up, True, "sr")
    R = _C._binning_hint[key]
    T = ((deep["W"] + 15) // 16) * ((deep["H"] + 15) // 16)
    assert R // T > 800 and R > 4 * key[1] * 1.25 + 1024          # step 1 did not fit and counted as "many big tiles"
    cam1, sc1, up1 = scenes.sensor_grid(**first)
    _compare(cam1, sc1, up1, True, "sr")
    T1 = ((first["W"] + 15) // 16) * ((first["H"] + 15) // 16)
    assert 0 < _C._binning_hint[(key[0], first["W"] * first["H"], first["W"], first["H"])] // T1 <= 800
    assert _C._binning_hint[key] == R                              # step 3 finds room
    _compare(cam, sc, up, True, "sr")
    assert _C._binning_hint[key] == R


def test_both_binning_paths():
    """HSR_SORT_IMPL=radix (read once per process: a child): emission in Gaussian order, stable radix passes over the tile bits, then the
    per-tile sort on segments that arrive in emission order — the LDS network on (depth, index) composites up to 2 048 entries, the block
    radix sort over the depth bytes alone beyond.  Equal depths stay in index order there only because every pass is stable."""
    code = ("import sys; sys.path[:0]=['hier-slam_amd','tests'];from test_gpu_depth_ties import _run_case;"
            "[_run_case(n) for n in ('first_frame','wide','deep','deep_65537')];print('ok')")
    env = dict(os.environ, HSR_SORT_IMPL="radix")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("name", ["first_frame", "wide"])
def test_legacy_accumulation(name):
    """'legacy' = atomics straight into the reference's six arrays (the all-VALU backward on quadrant lists): the same lists, read by
    another backward"""
    from diff_gaussian_rasterization import _C
    _C.set_backward_mode("legacy")
    try:
        _run_case(name)
    finally:
        _C.set_backward_mode("packed")
