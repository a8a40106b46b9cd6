"""CPU suite: the C oracle under general cameras.

tests/test_oracle.py pins the oracle against the float64 autograd restatement of tests/dense_ref.py through the identity and through
scenes.tilted_w2c, a turn about the y axis: in the column-major viewmatrix vm[1], vm[4], vm[6], vm[9] are then 0 and vm[5] is 1, and
projmatrix [1], [4], [7], [9] are 0.  An index or transposition error in those entries multiplies a zero or swaps two zeros, and the
oracle, the restatement and the kernels agree about the result.  Here the same comparisons run under the four cameras of scenes.CAMERAS
— every entry non-trivial, every entry large with a negative diagonal, x and y exchanged exactly, a pitch — at test_oracle.py's sizes,
and the oracle's per-Gaussian forward state (depths, means2D, conic) goes against the float64 values dense_render itself forms.

Bounds: test_oracle.py's (5e-6 on images, 2e-5 of the largest entry on gradients) wherever they hold.  Where the fp32 oracle sits further
from float64 than that, the case's bound is twice the distance measured (one fp32 evaluation is the floor; twice it leaves room for another
libm), written down in OVER and in the test's docstring.  Nothing may need more than 1e-4, the project's contract."""
import numpy as np
import pytest
import torch

import dense_ref as DR
import scenes
from harness import run_oracle

CAMS = list(scenes.CAMERAS)
IMG, GRAD, CONTRACT = 5e-6, 2e-5, 1e-4
MEASURED = []      # (case, quantity, distance): printed by every test, so that a run with -s shows the figures behind the bounds


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64).reshape(np.asarray(a).shape)
    return float(np.abs(a - b).max() / max(1e-12, np.abs(b).max()))


# cases over test_oracle.py's bound: (test, camera, ...) -> {quantity: distance measured, fp32 oracle against float64}; the bound is twice it
OVER = {
    ("cov", "skew140"): {"grad means3D": 2.140e-5},
}


def _bound(case, quantity, default):
    b = 2.0 * OVER[case][quantity] if quantity in OVER.get(case, {}) else default
    assert b <= CONTRACT, (case, quantity, b)
    return b


def _hold(case, quantity, distance, default):
    print("oracle vs float64  %-40s %-18s %.3e" % ("/".join(str(c) for c in case), quantity, distance))
    MEASURED.append((case, quantity, distance))
    assert distance < _bound(case, quantity, default), (case, quantity, distance)


def test_the_cameras_are_general():
    """the two skew cameras have no small entry (0.025 and 0.108 measured), every camera is a proper rotation to 1e-12, and between
    them no entry of the rotation that the kernels read is 0 or 1 in all cases — so a later edit cannot quietly hand back a trivial camera"""
    assert list(scenes.CAMERAS) == ["skew23", "skew140", "roll90", "pitch17"]
    for name, m in scenes.CAMERAS.items():
        assert m.shape == (4, 4) and m.dtype == np.float64 and np.array_equal(m[3], [0, 0, 0, 1]), name
        R = m[:3, :3]
        assert abs(np.linalg.det(R) - 1.0) <= 1e-12 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-12, name
    low = {n: float(np.abs(scenes.CAMERAS[n][:3, :3]).min()) for n in ("skew23", "skew140")}
    print("smallest |R entry|:", low)
    assert low["skew23"] >= 0.02 and low["skew140"] >= 0.02
    assert float(np.abs(scenes.CAMERAS["skew140"][:3, :3]).min()) >= 0.1 and (np.diag(scenes.CAMERAS["skew140"][:3, :3]) < 0).sum() == 2
    for n in ("skew23", "skew140"):
        assert (np.abs(scenes.CAMERAS[n][:3, 3]) > 0.05).all() and float(np.abs(np.abs(scenes.CAMERAS[n][:3, :3]) - 1).min()) > 0.004, n
    roll = scenes.CAMERAS["roll90"][:3, :3]
    assert np.abs(roll - np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]])).max() <= 1e-15      # x and y exchanged, one sign
    pitch = scenes.CAMERAS["pitch17"][:3, :3]
    assert abs(pitch[1, 2]) > 0.25 and abs(pitch[2, 1]) > 0.25 and np.array_equal(pitch[0], [1, 0, 0])
    # what the kernels read: the column-major viewmatrix and projmatrix of the camera tensors, in fp32
    for n in ("skew23", "skew140"):
        cam, _, _ = scenes.build(40, 36, 4, 0, w2c=scenes.CAMERAS[n])
        vm, pm = cam["viewmatrix"].reshape(-1).numpy(), cam["projmatrix"].reshape(-1).numpy()
        for i in (0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14):
            assert 0.02 <= abs(float(vm[i])) <= 0.999, (n, i, float(vm[i]))
        assert np.array_equal(vm[[3, 7, 11, 15]], [0, 0, 0, 1])
        assert (np.abs(pm) > 1e-3).all(), n


def test_build_without_a_camera_is_unchanged():
    """scenes.build's defaults: the y-turn, bit for bit what it was; a given camera replaces it for the tensors and for the placement"""
    from hsr_utils.camera import replica_intrinsics, setup_camera_tensors
    from hsr_utils.synthetic import make_scene
    k = replica_intrinsics(40, 36)
    cam, sc, up = scenes.build(40, 36, 60, 5, seed=3, kind="aniso", scale_mult=4.0)
    ref = setup_camera_tensors(40, 36, k, scenes.tilted_w2c())
    want = make_scene(60, 40, 36, 5, k, seed=3, kind="aniso", scale_mult=4.0, w2c=scenes.tilted_w2c())
    assert torch.equal(cam["viewmatrix"], ref["viewmatrix"]) and torch.equal(cam["projmatrix"], ref["projmatrix"])
    assert all(torch.equal(sc[n], want[n]) for n in want)
    m = scenes.CAMERAS["skew140"]
    cam2, sc2, up2 = scenes.build(40, 36, 60, 5, seed=3, kind="aniso", scale_mult=4.0, w2c=m)
    assert torch.equal(cam2["viewmatrix"], setup_camera_tensors(40, 36, k, m)["viewmatrix"])
    assert torch.equal(sc2["means3D"], make_scene(60, 40, 36, 5, k, seed=3, kind="aniso", scale_mult=4.0, w2c=m)["means3D"])
    assert all(torch.equal(up[n], up2[n]) for n in up) and torch.equal(sc["scales"], sc2["scales"])
    # the scene stands in front of the given camera: the same camera-space points, to rounding
    t = torch.cat([sc2["means3D"], torch.ones(60, 1)], 1) @ cam2["viewmatrix"].reshape(4, 4)
    t0 = torch.cat([sc["means3D"], torch.ones(60, 1)], 1) @ cam["viewmatrix"].reshape(4, 4)
    assert float((t - t0).abs().max()) < 1e-5 and float(t[:, 2].min()) > 0.4


def _forward_state(case, out, st, dout):
    """the oracle's depths, means2D and conic of visible Gaussians against the float64 values dense_render formed: depths relative to
    themselves, means2D in pixels relative to max(1, |coordinate|), the conic's three numbers relative to the row's largest"""
    vis = out["radii"] > 0
    assert vis.sum() >= 10
    s = dout["state"]
    d64, m64, c64 = s["depths"].numpy()[vis], s["means2D"].numpy()[vis], s["conic"].numpy()[vis]
    d32, m32, c32 = st.field("depths")[vis].astype(np.float64), st.field("means2D")[vis].astype(np.float64), \
        st.field("conic_opacity")[vis][:, :3].astype(np.float64)
    fd, fm, fc = (2.0 * v for v in FWD_MEASURED[case[1]])
    _hold(case, "state depths", float((np.abs(d32 - d64) / np.abs(d64)).max()), fd)
    _hold(case, "state means2D", float((np.abs(m32 - m64) / np.maximum(1.0, np.abs(m64))).max()), fm)
    _hold(case, "state conic", float((np.abs(c32 - c64) / np.abs(c64).max(axis=1, keepdims=True)).max()), fc)


# The forward state's distances, fp32 oracle against float64, as _forward_state forms them: per camera the largest over the three kinds
# (depths and means2D do not depend on the kind).  The tolerance is twice the figure.  means2D is the least exact: ndc2Pix forms
# ((p + 1) W - 1) / 2 from an ndc coordinate that may lie near -1, after a perspective division by w + 1e-7.
FWD_MEASURED = {
    #            depths     means2D    conic
    "skew23":   (8.504e-8, 7.497e-7, 8.319e-7),
    "skew140":  (1.382e-7, 3.979e-6, 8.323e-7),
    "roll90":   (4.409e-8, 1.254e-6, 1.757e-6),
    "pitch17":  (9.656e-8, 3.242e-6, 7.215e-7),
}


@pytest.mark.parametrize("kind,semantic,bg", [("aniso", True, (0.3, 0.6, 0.1)), ("slam", True, (0, 0, 0)), ("aniso", False, (0.0, 0.0, 0.0))],
                         ids=["aniso", "slam", "plain"])
@pytest.mark.parametrize("camera", CAMS)
def test_oracle_matches_float64_autograd(camera, kind, semantic, bg):
    """test_oracle.py's comparison of the same name, under each camera, and the forward state with it.
    Measured, fp32 oracle against float64 (largest image distance; largest gradient distance over its tensor's maximum), per kind:
        skew23    aniso 8.8e-7, 6.0e-7   slam 1.2e-6, 7.6e-7   plain 8.8e-7, 6.2e-7
        skew140   aniso 1.2e-6, 5.3e-7   slam 9.3e-7, 5.1e-7   plain 1.2e-6, 2.3e-6
        roll90    aniso 9.8e-7, 8.5e-7   slam 1.2e-6, 4.8e-7   plain 9.8e-7, 1.0e-6
        pitch17   aniso 1.1e-6, 5.3e-7   slam 1.2e-6, 1.1e-6   plain 1.1e-6, 8.4e-7
    n_contrib equal everywhere.  All within test_oracle.py's 5e-6 and 2e-5, which therefore hold unchanged.  The forward state: FWD_MEASURED."""
    W, H, K, P = 40, 36, 5, 60
    case = ("main", camera, kind if semantic else "plain")
    cam, sc, up = scenes.build(W, H, P, K if semantic else 0, seed=3, kind=kind, scale_mult=4.0, bg=bg, w2c=scenes.CAMERAS[camera])
    out, gr, st = run_oracle(cam, sc, up, semantic=semantic, threads=2)
    g = {n: v.numpy() for n, v in up.items()}
    dout, dgr = DR.dense_loss_and_grads(cam, sc, g, st.field("vals"), st.field("ranges"), semantic=semantic)
    assert int((st.field("n_contrib").reshape(H, W) != dout["n_contrib"].numpy()).sum()) == 0
    assert float(out["opacity"].max()) > 0.5      # the scene is in view under this camera
    for a, b in (("color", "color"), ("depth", "depth"), ("median_depth", "median"), ("opacity", "opacity"),
                 ("semantic", "semantic") if semantic else ("mask", "mask")):
        _hold(case, a, float(np.abs(out[a] - dout[b].detach().numpy()).max()), IMG)
    pairs = dict(means3D="means3D", scales="scales", rotations="rotations", opacities="opacities_ref", colors_precomp="colors")
    if semantic:
        pairs["semantics_precomp"] = "semantics"
    for a, b in pairs.items():
        _hold(case, "grad " + a, _rel(gr[a], dgr[b].numpy()), GRAD)
    _hold(case, "grad means2D", _rel(gr["means2D"][:, :2], dgr["ndc_delta"].numpy()), GRAD)
    _forward_state(case, out, st, dout)
    st.free()


@pytest.mark.parametrize("camera", CAMS)
def test_oracle_cov3d_precomp_matches_autograd(camera):
    """test_oracle.py's cov3D_precomp case (seed 8) under each camera.
    Measured, fp32 oracle against float64 (colour; grad cov3D_precomp; grad means3D):
        skew23    2.7e-7   2.5e-6   3.9e-7
        skew140   4.0e-7   4.1e-6   2.1e-5      <- over 2e-5: this case's bound for grad means3D is 2 x 2.140e-5 = 4.3e-5 (OVER)
        roll90    3.3e-7   2.6e-7   1.3e-6
        pitch17   3.0e-7   1.0e-6   6.1e-7
    Everything else is held to test_oracle.py's 5e-6 and 2e-5."""
    W, H, K, P = 40, 36, 4, 50
    case = ("cov", camera)
    cam, sc, up = scenes.build(W, H, P, K, seed=8, kind="aniso", scale_mult=4.0, w2c=scenes.CAMERAS[camera])
    sc["cov3D_precomp"] = scenes.cov3d_from_scene(sc)
    out, gr, st = run_oracle(cam, sc, up, semantic=True, variant="cov", extra=sc, threads=2)
    g = {n: v.numpy() for n, v in up.items()}
    dout, dgr = DR.dense_loss_and_grads(cam, sc, g, st.field("vals"), st.field("ranges"), use_cov3d=True)
    assert int((st.field("n_contrib").reshape(H, W) != dout["n_contrib"].numpy()).sum()) == 0
    _hold(case, "color", float(np.abs(out["color"] - dout["color"].detach().numpy()).max()), IMG)
    _hold(case, "grad cov3D_precomp", _rel(gr["cov3D_precomp"], dgr["cov3D"].numpy()), GRAD)
    _hold(case, "grad means3D", _rel(gr["means3D"], dgr["means3D"].numpy()), GRAD)
    st.free()


@pytest.mark.parametrize("deg", [1, 3])
@pytest.mark.parametrize("camera", CAMS)
def test_oracle_sh_matches_float64_autograd(camera, deg):
    """test_oracle.py's SH comparison (degrees 1 and 3) under each camera: campos = inverse(w2c)[:3, 3] is no longer a y-turn's, and
    the view-direction term of grad means3D has all three components live.
    Measured, fp32 oracle against float64 (largest of SH colour and image; largest gradient distance), degree 1 and degree 3:
        skew23    2.9e-7, 1.6e-6   2.8e-7, 1.4e-6
        skew140   3.0e-7, 7.2e-7   2.2e-7, 9.2e-7
        roll90    2.5e-7, 1.9e-6   3.0e-7, 1.1e-6
        pitch17   2.2e-7, 1.8e-6   3.4e-7, 2.4e-6
    All within test_oracle.py's 2e-6 (SH colour), 5e-6 and 2e-5, which hold unchanged."""
    W, H, K, P = 40, 36, 4, 60
    case = ("sh", camera, deg)
    m = scenes.CAMERAS[camera]
    cam, sc, up = scenes.build(W, H, P, K, seed=4, kind="aniso", scale_mult=4.0, w2c=m)
    assert np.abs(cam["campos"].numpy() - (-m[:3, :3].T @ m[:3, 3])).max() < 1e-6
    cam["sh_degree"] = deg
    shs = scenes.random_sh(P, 16, seed=9)
    shs[::5, 0, :] -= 3.2
    shs[1::7, 0, 1] -= 3.2
    out, gr, st = run_oracle(cam, sc, up, semantic=True, extra={"shs": shs}, threads=2)
    g = {n: v.numpy() for n, v in up.items()}
    dout, dgr = DR.dense_loss_and_grads_sh(cam, sc, shs.numpy(), deg, g, st.field("vals"), st.field("ranges"))
    vis = out["radii"] > 0
    _hold(case, "rgb", float(np.abs(st.field("rgb")[vis] - dgr["colors_value"].numpy()[vis]).max()), 2e-6)
    clamped = st.field("clamped").astype(bool)
    assert clamped[vis].any() and not clamped[vis].all()
    assert np.array_equal(clamped[vis], (dgr["colors_value"].numpy()[vis] == 0))
    _hold(case, "color", float(np.abs(out["color"] - dout["color"].detach().numpy()).max()), IMG)
    nb = (deg + 1) ** 2
    _hold(case, "grad shs", _rel(gr["shs"][:, :nb], dgr["shs"].numpy()[:, :nb]), GRAD)
    assert not gr["shs"][:, nb:].any()
    assert float(np.abs(gr["shs"][clamped[:, 0], :, 0]).max()) == 0
    for a, b in dict(means3D="means3D", scales="scales", rotations="rotations", opacities="opacities_ref",
                     semantics_precomp="semantics").items():
        _hold(case, "grad " + a, _rel(gr[a], dgr[b].numpy()), GRAD)
    st.free()
