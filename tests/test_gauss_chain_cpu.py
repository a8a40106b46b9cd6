"""CPU: the oracle's per-Gaussian chain as an entry point (hsro_gauss_chain), and the case table of tests/gauss_chain_cases.py held to
the regimes its Gaussians are named for — on the oracle's forward state, so that the table cannot drift away from the branches
tests/test_gpu_gauss_chain.py runs it for."""
import numpy as np
import pytest

import gauss_chain_cases as G
import oracle_lib as O
from harness import variant_kwargs

F32 = np.float32
CHAIN_KEYS = ("means3D", "cov3D_precomp", "shs", "scales", "rotations")


def _forward(case, precision="f32", semantic=True):
    kw = variant_kwargs(case.sc, case.variant, case.extra)
    if semantic:
        kw["semantics_precomp"] = case.sc["semantics_precomp"]
    out, st = O.forward(case.cam, case.sc["means3D"], case.sc["opacities"], precision=precision, **kw)
    return out, st, kw


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("name", ["directed", "directed_mod1.7", "directed_cov", "directed_sh3", "random_100x70_off_centre_sh3"])
def test_chain_on_the_backward_s_own_sums_is_the_backward_bit_for_bit(name, precision):
    case = G.CASES[name]()
    out, st, kw = _forward(case, precision)
    try:
        g = {n: v.numpy() for n, v in case.up.items()}
        gr = O.backward(st, case.cam, case.sc["means3D"], g, median_rule="forward", **kw)
        ch = O.gauss_chain(st, case.cam, case.sc["means3D"], gr, **kw)
        assert gr["means3D"].dtype == (np.float64 if precision == "f64" else np.float32)
        assert np.abs(gr["means3D"]).max() > 0 and np.abs(gr["cov3D_precomp"]).max() > 0
        for key in CHAIN_KEYS:
            assert ch[key].dtype == gr[key].dtype and ch[key].shape == gr[key].shape, key
            assert np.array_equal(ch[key].view(np.uint8), gr[key].view(np.uint8)), key
        culled = out["radii"] <= 0
        assert culled.any()
        for key in CHAIN_KEYS:
            assert not ch[key][culled].any(), key
    finally:
        st.free()


def test_chain_is_linear_in_its_input_groups():
    """what the GPU test's scale rests on: the chain run with one input group at a time adds up to the chain run with all of them"""
    case = G.CASES["directed_sh3"]()
    out, st, kw = _forward(case, "f64")
    try:
        rng = np.random.default_rng(5)
        P = st.P
        full = dict(means2D=rng.standard_normal((P, 3)), conic=rng.standard_normal((P, 4)), depths=rng.standard_normal((P, 1)),
                    colors_precomp=rng.standard_normal((P, 3)))
        t = O.gauss_chain(st, case.cam, case.sc["means3D"], full, **kw)
        parts = [O.gauss_chain(st, case.cam, case.sc["means3D"], {n: (v if n == keep else np.zeros_like(v)) for n, v in full.items()}, **kw)
                 for keep in full]
        for key in CHAIN_KEYS:
            s = sum(p[key] for p in parts)
            scale = sum(np.abs(p[key]) for p in parts)
            assert np.all(np.abs(s - t[key]) <= 1e-13 * scale + 1e-300), key
    finally:
        st.free()


def _side(v, lim):
    """which side of the clamp the kernels' test (t < -lim || t > lim) puts v / 1.0f on; "on": exactly at the limit, not clamped"""
    v = abs(F32(v) / F32(1.0))
    return "on" if v == lim else ("out" if v > lim else "in")


def test_every_directed_gaussian_is_in_the_regime_it_is_named_for():
    info = G.directed_info()
    assert {d["index"] for d in info.values()} >= {0, 63, 64, 255, 256, 257, 599}
    assert {d["group"] for d in info.values()} == {"near", "clamp", "radius", "rot_scale", "opacity", "cov"}
    case = G.CASES["directed"]()
    out, st, _ = _forward(case)
    try:
        radii, touched = out["radii"], st.field("tiles_touched")
        means2D, conic, depths = st.field("means2D"), st.field("conic_opacity"), st.field("depths")
        m = case.sc["means3D"].numpy()
        limx, limy = G.limits(case.cam)
        # cov2D = 0.3 I: det = 0.3f * 0.3f, conic = 0.3f * (1 / det), and mid^2 - det = 0 < 0.1
        floor_conic = F32(0.3) * (F32(1.0) / (F32(0.3) * F32(0.3)))
        for name, d in info.items():
            i = d["index"]
            assert (radii[i] > 0) == d["visible"], name
            if d["visible"]:
                assert depths[i] == m[i, 2], name                  # identity w2c: the view depth is z, bit for bit
            if "radius" in d:
                assert radii[i] == d["radius"], name
            if "tiles" in d:
                assert touched[i] == d["tiles"], (name, int(touched[i]))
            if "clamp" in d:
                assert (_side(m[i, 0], limx), _side(m[i, 1], limy)) == d["clamp"], name
                assert touched[i] >= 1, name                       # outside the clamp, yet on the screen
            if "floor" in d:
                a, b, c = (float(v) for v in conic[i, :3])
                det = 1.0 / (a * c - b * b)                        # cov2D + 0.3 I back from its inverse, in double
                cx, cz = c * det, a * det
                assert ((0.5 * (cx + cz)) ** 2 - det < 0.1) == d["floor"], name
                if d["floor"]:
                    assert conic[i, 0] == floor_conic and conic[i, 2] == floor_conic and abs(conic[i, 1]) < 1e-8, name
        # near: the three neighbouring floats around 0.2f
        z = [m[info[n]["index"], 2] for n in ("near_below", "near_at", "near_above")]
        assert z[1] == F32(0.2) and np.nextafter(z[1], F32(0)) == z[0] and np.nextafter(z[1], F32(1)) == z[2]
        # clamp: on / in / out are neighbouring floats, far is 1.6 times the limit
        for ax, lim, tag in ((0, limx, "x"), (1, limy, "y")):
            on, inn, outt, far = (abs(m[info["clamp_%s_%s" % (tag, n)]["index"], ax]) for n in ("on", "in", "out" if tag == "y" else "far", "far"))
            assert on == lim and np.nextafter(lim, F32(0)) == inn and far == F32(1.6) * lim
            if tag == "y":
                assert np.nextafter(lim, F32(9)) == outt
        assert m[0, 0] == np.nextafter(limx, F32(9))               # clamp_x_out stands at index 0
        # rect: the centres sit exactly where (p - r) / 16 and ((p + r) + 16 - 1) / 16 are integers
        assert tuple(means2D[info["rect_min_edge"]["index"]]) == (19.0, 19.0)
        assert tuple(means2D[info["rect_max_edge"]["index"]]) == (30.0, 14.0)
        assert means2D[info["rect_first_column"]["index"], 0] == -2.0 and means2D[info["rect_last_column"]["index"], 0] == 65.5
        lo = np.nextafter(F32(19.0), F32(0))
        assert (F32(19.0) - F32(3)) / F32(16) == F32(1) and int((lo - F32(3)) / F32(16)) == 0
        assert ((F32(30.0) + F32(3)) + F32(16) - F32(1)) / F32(16) == F32(3) and ((F32(14.0) + F32(3)) + F32(16) - F32(1)) / F32(16) == F32(2)
        assert ((F32(-2.0) + F32(3)) + F32(16) - F32(1)) / F32(16) == F32(1)
        e = info["rect_empty"]["index"]
        assert m[e, 2] == 1.0 and radii[e] == 0                    # a visible depth, culled by its empty rectangle
        # opacity: visible, and no pixel takes them (alpha < 1/255 everywhere): the tile pass adds nothing into their rows
        g = {n: v.numpy() for n, v in case.up.items()}
        kw = variant_kwargs(case.sc, case.variant, case.extra)
        gr = O.backward(st, case.cam, m, g, median_rule="forward", semantics_precomp=case.sc["semantics_precomp"], **kw)
        op = [d["index"] for d in info.values() if d["group"] == "opacity"]
        assert len(op) == 3 and [float(case.sc["opacities"][i]) for i in op] == [0.0, 1.0 / 512, float(F32(1.0) / F32(255.0))]
        for key in ("means2D", "conic", "opacities", "colors_precomp", "semantics_precomp", "depths", "means3D", "scales", "rotations"):
            assert not gr[key][op].any(), key
        assert not st.field("tie_gaussians")[op].any()             # and none of them within ulps of the 1/255 threshold
        # rot_scale: what the table says of the quaternions and scales
        q = case.sc["rotations"].numpy()
        s = case.sc["scales"].numpy()
        assert not q[info["quat_zero"]["index"]].any()
        assert abs(np.linalg.norm(q[info["quat_norm_2"]["index"]]) - 2.0) < 1e-6 and abs(np.linalg.norm(q[info["quat_norm_half"]["index"]]) - 0.5) < 1e-6
        assert sorted(s[info["scale_axis_0"]["index"]])[0] == 0.0
        assert s[info["needle_30"]["index"]].max() / s[info["needle_30"]["index"]].min() == pytest.approx(30.0)
        assert s[info["needle_300"]["index"]].max() / s[info["needle_300"]["index"]].min() == pytest.approx(300.0)
    finally:
        st.free()


def test_cov3d_variant_has_a_row_culled_by_det_equal_zero_and_one_with_a_tiny_det():
    info = G.directed_info()
    case = G.CASES["directed_cov"]()
    i0, i1 = info["cov_det0"]["index"], info["cov_det1e-4"]["index"]

    def radii_and_conic(cov):
        out, st = O.forward(case.cam, case.sc["means3D"], case.sc["opacities"], colors_precomp=case.sc["colors_precomp"], cov3D_precomp=cov)
        c = st.field("conic_opacity")
        st.free()
        return out["radii"], c
    cov = case.extra["cov3D_precomp"].numpy().copy()
    assert cov[i0, 0] * cov[i0, 3] < cov[i0, 1] ** 2               # not positive semi-definite
    radii, conic = radii_and_conic(cov)
    assert case.sc["means3D"][i0, 2] == 1.0 and radii[i0] == 0     # a visible depth in the middle of the image: culled by det == 0
    for step in (F32(0), F32(1)):                                  # the off-diagonal entry one float lower or higher: det != 0, kept
        c2 = cov.copy()
        c2[i0, 1] = np.nextafter(cov[i0, 1], step)
        assert radii_and_conic(c2)[0][i0] > 0
    assert radii[i1] > 0
    a, b, c = (float(v) for v in conic[i1, :3])
    det = 1.0 / (a * c - b * b)
    assert 0.9e-4 < det < 1.1e-4, det
    assert 1.0 / (det * det + 1e-7) > 8e6                          # denom2inv: large, finite


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_sh_variants_have_clamped_channels_and_one_at_zero_that_is_not(deg):
    case = G.CASES["directed_sh%d" % deg]()
    out, st, _ = _forward(case)
    try:
        vis = out["radii"] > 0
        clamped, rgb = st.field("clamped"), st.field("rgb")
        i = G.SH_GAUSSIAN
        assert vis[i]
        assert clamped[i, 1] == 1 and rgb[i, 1] == 0.0
        assert clamped[i, 2] == 0 and rgb[i, 2] == 0.0 and not np.signbit(rgb[i, 2])     # 0.0f after the + 0.5f: r < 0 is false
        assert clamped[i, 0] == 0 and rgb[i, 0] > 0.0
        assert int(clamped[vis].sum()) >= 50 and int((clamped[vis] == 0).sum()) >= 1000
    finally:
        st.free()


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_clamp_zeroes_the_mean_gradient_of_a_clamped_axis_and_of_no_other(precision):
    """identity w2c and a conic-only cotangent: dL_dmean3D.x = x_grad_mul * (...) exactly — 0 outside the clamp, not 0 on the limit"""
    info = G.directed_info()
    case = G.CASES["directed"]()
    out, st, kw = _forward(case, precision)
    try:
        P = st.P
        rng = np.random.default_rng(3)
        sums = dict(means2D=np.zeros((P, 3)), conic=rng.standard_normal((P, 4)), depths=np.zeros((P, 1)), colors_precomp=np.zeros((P, 3)))
        ch = O.gauss_chain(st, case.cam, case.sc["means3D"], sums, **kw)
        seen = set()
        for name, d in info.items():
            if "clamp" not in d:
                continue
            g = ch["means3D"][d["index"]]
            for ax, side in enumerate(d["clamp"]):
                seen.add((ax, side))
                if side == "out":
                    assert g[ax] == 0.0, (name, ax, g)
                else:
                    assert g[ax] != 0.0, (name, ax, g)
            assert g[2] != 0.0, name
        assert seen == {(0, "in"), (0, "on"), (0, "out"), (1, "in"), (1, "on"), (1, "out")}
    finally:
        st.free()
