"""-m gpu: the per-Gaussian chain of the backward (hsr_backward_pre.hip: dL_dconic -> cov2D -> cov3D -> scale / quaternion, mean2D and depth ->
mean3D, SH backward) and the float state hsr_preprocess.hip writes for it (cov3D, the SH colours, the clamp flags), apart from the tile sums.

Every other comparison of these outputs (test_gpu_parity.py, test_gpu_fuzz.py, test_gpu_bwd_unpack.py) feeds the chain with sums the tile
kernel accumulated with fp32 atomics and compares with an oracle that summed in double: the chain's outputs inherit the arrival-order noise,
and scales / rotations / cov3D are held element-wise only down to half of the tensor's largest entry.  Here the backward is called straight
at the C ABI with buffers for the intermediates too (dL_dconic, dL_ddepth), and the ORACLE'S chain (oracle_lib.gauss_chain) is run on the
DEVICE'S OWN intermediates: the chain is linear in them, the atomics drop out, and what is left is one chain evaluated twice in fp32,
without contraction (csrc/Makefile: hsr_backward_pre.o is built with -ffp-contract=off for exactly this).

The bound.  d: the device's output, o: the fp32 oracle's chain, t: the float64 chain, all on the device's intermediates.
  1. every element of d bit-equal to o.
  2. an element that is not falls to the second tier.  Scale of row i of a tensor: s_i = max_j sum_paths |t^path_ij|, the paths being the
     float64 chain run with one input group alone (conic, mean2D, depth, colour) — they add up to t, and their absolute sum is what the rounding
     error of the row scales with.  E(x) = max_ij |x_ij - t_ij| / s_i.  Required: E(d) <= 2 E(o) per tensor and case (the margin two fp32
     evaluations of one chain get elsewhere in this suite), and at most 1 % of a tensor's elements of visible Gaussians in the second tier.
Printed per case and tensor: elements compared, elements not bit-equal, E(d), E(o).

Cases: tests/gauss_chain_cases.py (tests/test_gauss_chain_cpu.py holds the table to its regimes).  Each runs with packed rows at K = 0 (a
row read from global memory), at K = 26 (rows staged in LDS) and in the legacy accumulation mode."""
import ctypes as C

import numpy as np
import pytest
import torch

import gauss_chain_cases as G
import oracle_lib as O
from harness import device_state, variant_kwargs
from test_gpu_parity import _compare_integers

pytestmark = pytest.mark.gpu

MODES = ("packed_k0", "packed_k26", "legacy_k26")
CHAIN = ("means3D", "cov3D_precomp", "scales", "rotations", "shs")
TIER2_SHARE = 0.01

_ORACLE = {}     # case name -> the oracle's forward (fp32 and float64 states): computed once, shared by the modes


def _oracle(name, case):
    if name not in _ORACLE:
        kw = variant_kwargs(case.sc, case.variant, case.extra)
        out_o, st_o = O.forward(case.cam, case.sc["means3D"], case.sc["opacities"], **kw)
        _, st_t = O.forward(case.cam, case.sc["means3D"], case.sc["opacities"], precision="f64", **kw)
        _ORACLE[name] = (out_o, st_o, st_t, kw)
    return _ORACLE[name]


def _device(case, semantic):
    """forward through the glue, backward straight at the C ABI into NaN-filled buffers for EVERY output; returns (radii, state, gradients)"""
    from diff_gaussian_rasterization import _C, _abi
    dev = torch.device("cuda:0")
    cam, sc = case.cam, case.sc
    P, W, H = int(sc["means3D"].shape[0]), int(cam["image_width"]), int(cam["image_height"])
    K = int(sc["semantics_precomp"].shape[1]) if semantic else 0
    kw = variant_kwargs(sc, case.variant, case.extra)
    none = torch.Tensor([])
    t = lambda v: v.to(dev).float().contiguous()
    g = lambda n: t(kw[n]) if n in kw else none
    bg, vm, pm, cp = (t(cam[n]) for n in ("bg", "viewmatrix", "projmatrix", "campos"))
    means3D, opac = t(sc["means3D"]), t(sc["opacities"])
    colors, shs, scales, rots, cov = g("colors_precomp"), g("shs"), g("scales"), g("rotations"), g("cov3D_precomp")
    tail = (opac, scales, rots, float(cam["scale_modifier"]), cov, vm, pm, float(cam["tanfovx"]), float(cam["tanfovy"]), H, W, shs,
            int(cam["sh_degree"]), cp, False, False)
    if semantic:
        sem = t(sc["semantics_precomp"])
        R, _, _, _, _, _, radii, geom, binning, img = _C.rasterize_gaussians_semantic(bg, means3D, colors, sem, *tail)
    else:
        R, _, _, _, _, _, radii, geom, binning, img = _C.rasterize_gaussians(bg, means3D, colors, *tail)
    R = int(R)
    state = device_state(geom, binning, img, P, W, H, R)
    M = int(shs.shape[1]) if shs.numel() else 0
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
    out = dict(means2D=nan(P, 3), conic=nan(P, 4), opacities=nan(P, 1), colors_precomp=nan(P, 3), semantics_precomp=nan(P, K),
               depths=nan(P, 1), means3D=nan(P, 3), cov3D_precomp=nan(P, 6), shs=nan(P, M, 3))
    if scales.numel():
        out["scales"], out["rotations"] = nan(P, 3), nan(P, 4)
    plan = _abi.hsr_backward_plan()
    assert _abi.lib.hsr_plan_backward(P, K, 0, _abi.HSR_SCRATCH_AS_PLANNED, C.byref(plan)) >= 0
    nscratch = int(plan.scratch_bytes)
    scratch = torch.full((nscratch,), 0xFF, dtype=torch.uint8, device=dev) if nscratch else None      # rows of NaN
    p = lambda x: None if (x is None or x.numel() == 0) else x.data_ptr()
    po = lambda n: p(out.get(n))
    up = {n: t(v) for n, v in case.up.items()}
    stream = torch.cuda.current_stream(dev).cuda_stream
    head = (bg.data_ptr(), W, H, p(means3D), p(shs), p(colors))
    mid = (p(scales), float(cam["scale_modifier"]), p(rots), p(cov), p(vm), p(pm), p(cp), float(cam["tanfovx"]), float(cam["tanfovy"]),
           p(radii), p(geom), p(binning), p(img))
    back = (po("means3D"), po("cov3D_precomp"), po("shs"), po("scales"), po("rotations"), p(scratch), nscratch, 0, stream)
    if semantic:
        rc = _abi.lib.hsr_backward_semantic(P, int(cam["sh_degree"]), M, K, R, *head, p(sem), *mid,
                                            p(up["color"]), p(up["semantic"]), p(up["depth"]), p(up["median"]), p(up["opacity"]),
                                            po("means2D"), po("conic"), po("opacities"), po("colors_precomp"), po("semantics_precomp"),
                                            po("depths"), *back)
    else:
        rc = _abi.lib.hsr_backward(P, int(cam["sh_degree"]), M, R, *head, *mid,
                                   p(up["color"]), p(up["depth"]), p(up["median"]), p(up["opacity"]),
                                   po("means2D"), po("conic"), po("opacities"), po("colors_precomp"), po("depths"), *back)
    if rc < 0:
        _abi.fail(rc, "hsr_backward")
    torch.cuda.synchronize()
    return radii.cpu().numpy(), state, {n: v.cpu().numpy() for n, v in out.items()}, int(plan.accumulation)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(name, case, mode, directed):
    from diff_gaussian_rasterization import _C
    semantic = mode != "packed_k0"
    out_o, st_o, st_t, kw = _oracle(name, case)
    if mode.startswith("legacy"):
        _C.set_backward_mode("legacy")
    try:
        radii, st_g, gr, accumulation = _device(case, semantic)
    finally:
        _C.set_backward_mode("packed")
    assert accumulation == (2 if mode.startswith("legacy") else 0)
    P = radii.shape[0]
    sh = "shs" in kw
    # ---- the forward's state: integers and the fp32 state behind them as everywhere; cov3D, the SH colours and the clamp flags too ----
    _compare_integers(dict(radii=radii), st_g, out_o, st_o, own_cov3D=case.variant != "cov")
    vis = out_o["radii"] > 0
    assert vis.any() and (not directed or P < 64 or not vis.all())      # the directed scene has culled rows between visible ones
    if sh:
        assert np.array_equal(st_g["clamped"][vis], st_o.field("clamped")[vis]), "clamped"
        assert np.array_equal(_bits(st_g["rgb"][vis]), _bits(st_o.field("rgb")[vis])), "rgb"
    # ---- every element of every output written; zeros where the rules say zero ----
    for n, v in gr.items():
        assert not np.isnan(v).any(), "%s: %d elements were not written (or are NaN)" % (n, int(np.isnan(v).sum()))
        assert np.isfinite(v).all(), n
        assert not v[~vis].any(), "%s: a culled Gaussian has a gradient" % n
    assert not gr["means2D"][:, 2].any() and not gr["conic"][:, 2].any()
    if sh:
        active = (int(case.cam["sh_degree"]) + 1) ** 2
        assert not gr["shs"][:, active:, :].any(), "dL_dsh above the active degree"
        cl = st_o.field("clamped").astype(bool)
        assert (cl & vis[:, None]).sum() > 0
        assert not np.transpose(gr["shs"], (0, 2, 1))[cl].any(), "dL_dsh of a clamped channel"
        assert np.abs(gr["shs"][:, :active, :]).max() > 0
    if directed:
        info = G.directed_info()
        op = [d["index"] for d in info.values() if d["group"] == "opacity" and d["index"] < P]
        for n, v in gr.items():
            assert not v[op].any(), "%s: a Gaussian that no pixel takes has a gradient" % n
        if op:
            assert vis[op].all()
    # ---- the chain alone: the oracle's, on the device's own intermediates ----
    sums = {n: gr[n] for n in ("means2D", "conic", "depths", "colors_precomp")}
    args = (case.cam, case.sc["means3D"])
    o = O.gauss_chain(st_o, *args, sums, **kw)
    t = O.gauss_chain(st_t, *args, sums, **kw)
    paths = [O.gauss_chain(st_t, *args, {n: (v if n == keep else np.zeros_like(v)) for n, v in sums.items()}, **kw) for keep in sums]
    failures = []
    for key in CHAIN:
        if key not in gr or gr[key].size == 0:
            continue
        d_, o_, t_ = (np.asarray(x[key]).reshape(P, -1) for x in (gr, o, t))
        assert o_.dtype == np.float32 and t_.dtype == np.float64 and d_.dtype == np.float32
        s = np.max(sum(np.abs(pth[key].reshape(P, -1)) for pth in paths), axis=1, keepdims=True)

        def E(x):
            err = np.abs(x.astype(np.float64) - t_)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(err == 0, 0.0, err / s)       # a row of scale 0 has t = 0: anything but 0 there is infinitely far
            return float(r.max())
        ne = _bits(d_) != _bits(o_)
        n_cmp, n_ne = int(vis.sum()) * d_.shape[1], int(ne[vis].sum())
        assert not ne[~vis].any()
        Ed, Eo = E(d_), E(o_)
        print("gauss_chain %-30s %-10s %-14s compared %6d  not bit-equal %5d  E(d) %.3e  E(o) %.3e" % (name, mode, key, n_cmp, n_ne, Ed, Eo))
        assert np.abs(t_[vis]).max() > 0, key
        if n_ne:
            if not (np.isfinite(Ed) and Ed <= 2.0 * Eo):
                failures.append("%s: E(d) = %.3e > 2 E(o) = %.3e (%d of %d elements not bit-equal)" % (key, Ed, 2.0 * Eo, n_ne, n_cmp))
            if n_ne > TIER2_SHARE * n_cmp:
                failures.append("%s: %d of %d elements are not bit-equal to the fp32 oracle's chain (more than 1 %%)" % (key, n_ne, n_cmp))
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(G.CASES))
def test_chain_and_its_state_against_the_oracle_on_the_device_s_own_sums(name, mode):
    _check(name, G.CASES[name](), mode, name.startswith("directed"))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_prefix_of_the_directed_scene_at_the_block_seams(n):
    """a block of one Gaussian, one short of a block, a whole block, a block and one: the seams of the outputs the unpack tests do not look
    at (dL_dmean3D, dL_dcov3D, dL_dscale, dL_drot)"""
    _check("directed[:%d]" % n, G.prefix(n), "packed_k26", True)
