"""CPU suite for the reference pin of frame prep, the camera mirror and the gradient-driven densify: what this repository's CPU-side
restatements (oracle/frame_prep_oracle.py, hsr_utils/camera.py, tests/test_gpu_densify._densify_stepwise) compute against what the
reference's own functions returned (tests/golden/slam_helpers/*.npz, written by tests/golden/make_slam_helpers_golden.py).  The kernels
meet the same fixtures in tests/test_gpu_frame_prep.py and tests/test_gpu_densify.py.

Figures of this suite on the fixtures (fp32 oracle forward / float64 oracle backward against the reference's fp32 values): forward within
FWD_RTOL / FWD_ATOL everywhere, gradients at most 1.2e-6 of a tensor's largest entry (bound BWD_TOL = 1e-4: the fixture is an fp32 autograd
result).  With the oracle as it was before F.normalize's eps branch was written into it, the six edge cases fail (NaN for the all-zero
quaternion row, 1e18 where the reference has 1e12 for the row of norm 5e-20)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import frame_prep_oracle as O  # noqa: E402
import slam_helpers_fixture as F  # noqa: E402


# ---------------------------------------------------------------- frame prep ----------------------------------------------------------------
def test_the_fixture_holds_the_cases_the_kernels_can_get_wrong():
    names = F.frame_prep_cases()
    cases = [F.frame_prep_case(n) for n in names]
    seen = {(c["builder"], c["S"], c["P"]) for c in cases if not c["edge"]}
    for b in ("rendervar", "semantic", "silhouette", "depthsil"):
        for S in (1, 3):
            assert (b, S, 1) in seen and (b, S, 257) in seen
    assert {c["P"] for c in cases} >= {1, 64, 257, 1025}
    assert {c["time_idx"] for c in cases} >= {0, 5} and all(c["inputs"]["cam_trans"].shape == (1, 3, 6) for c in cases)
    assert {(c["gaussians_grad"], c["camera_grad"]) for c in cases} == {(True, True), (True, False), (False, True), (False, False)}
    for c in cases:                               # the pose quaternion is never a unit one
        q = c["inputs"]["cam_unnorm_rots"][0, :, c["time_idx"]]
        assert abs(float(np.sqrt((q.astype(np.float64) ** 2).sum())) - 1.0) > 1e-2
    edge = F.frame_prep_case("edge_semantic_S1")
    norms = np.sqrt((edge["inputs"]["unnorm_rotations"][:4].astype(np.float64) ** 2).sum(axis=1))
    assert norms[0] == 0 and norms[1] < 1e-19 and 1e-13 < norms[2] < F.EPS < norms[3] < 1e-11
    assert edge["inputs"]["logit_opacities"][4, 0] == 90 and edge["inputs"]["logit_opacities"][5, 0] == -90
    assert edge["inputs"]["log_scales"].min() == -90 and edge["inputs"]["log_scales"].max() == 40


@pytest.mark.parametrize("name", F.frame_prep_cases())
def test_frame_prep_oracle_matches_the_reference(name):
    c = F.frame_prep_case(name)
    with np.errstate(all="ignore"):
        fo = O.forward(**c["inputs"], time_idx=c["time_idx"], rot_source=c["rot_source"], w2c=c["w2c"])
        got = F.oracle_backward(O, c)
    assert set(c["out"]) - {"sil_color"} == set(fo)
    for k in fo:
        F.assert_forward("%s %s" % (name, k), fo[k], c["out"][k])
    if c["builder"] == "silhouette":
        assert (c["out"]["sil_color"][:, 0] == 1).all() and not c["out"]["sil_color"][:, 1:].any()
    worst = F.check_gradients(c, got)
    print("%-28s oracle (float64) vs reference (fp32 autograd): largest gradient distance %.2e of the tensor's maximum" % (name, worst))


@pytest.mark.parametrize("name", ["edge_semantic_S1", "edge_pose_semantic_S1"])
def test_rows_below_eps_get_g_over_eps(name):
    """F.normalize's clamp passes no gradient: below eps the adjoint is g / eps, with no projection term, and finite at |u| = 0"""
    c = F.frame_prep_case(name)
    want = F.expected_below_eps_rows(c)
    np.testing.assert_allclose(c["grads"]["unnorm_rotations"][:3], want, rtol=1e-6)            # the reference's own rows
    assert np.abs(want).min() > 1e10
    with np.errstate(all="ignore"):
        got = F.oracle_backward(O, c)["unnorm_rotations"]
    np.testing.assert_allclose(got[:3], want, rtol=1e-6)


# ------------------------------------------------------------------ camera ------------------------------------------------------------------
def _camera_cases(kind):
    return sorted({k.split("/")[1] if kind == "setup" else "/".join(k.split("/")[1:3]) for k in F.load("camera.npz") if k.startswith(kind + "/")})


@pytest.mark.parametrize("name", _camera_cases("setup"))
def test_setup_camera_tensors_is_bit_equal_to_the_reference(name):
    from hsr_utils.camera import setup_camera_tensors
    z = F.load("camera.npz")
    i = lambda k: z["setup/%s/in/%s" % (name, k)]
    cam = setup_camera_tensors(int(i("w")), int(i("h")), i("k"), i("w2c"), near=float(i("near")), far=float(i("far")))
    for k in ("viewmatrix", "projmatrix", "campos", "bg"):
        want = z["setup/%s/out/%s" % (name, k)]
        got = cam[k].numpy()
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), k
    for k in ("tanfovx", "tanfovy", "image_height", "image_width", "scale_modifier", "sh_degree", "prefiltered", "debug"):
        want = z["setup/%s/out/%s" % (name, k)]
        assert cam[k] == want and np.asarray(cam[k]).dtype.kind == want.dtype.kind, (k, cam[k], want)
    assert set(cam) == {"viewmatrix", "projmatrix", "campos", "bg", "tanfovx", "tanfovy", "image_height", "image_width", "scale_modifier",
                        "sh_degree", "prefiltered", "debug"}


@pytest.mark.parametrize("name", _camera_cases("scale"))
def test_scale_intrinsics_is_bit_equal_to_the_reference(name):
    from hsr_utils.camera import scale_intrinsics
    z = F.load("camera.npz")
    key = "scale/" + name
    arr, want = z[key + "/in"], z[key + "/out"]
    is_tensor = bool(z[key + "/out_is_tensor"])
    assert is_tensor == name.startswith("tensor")
    src = torch.tensor(arr) if is_tensor else arr.copy()
    got = scale_intrinsics(src, float(z[key + "/h_ratio"]), float(z[key + "/w_ratio"]))
    assert torch.is_tensor(got) == is_tensor
    assert np.array_equal(np.asarray(src), arr)                                              # the input is not written to
    got = got.numpy() if is_tensor else got
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(got, arr.astype(np.float32))


# ------------------------------------------------------------------ densify -----------------------------------------------------------------
def test_the_densify_fixture_holds_the_cases():
    z = F.load("densify_gradient.npz")
    counts = {}
    for name in F.densify_cases():
        params, variables, opt, it, dd, draw, exp = F.densify_case(name)
        counts[name] = (params["means3D"].shape[0], params["log_scales"].shape[1], exp["param/means3D"].shape[0],
                        0 if draw is None else draw.shape[0])
        assert "timestep" not in variables and dd["num_to_split_into"] == 2
        assert all(float(opt.state[p]["step"]) == 2 for p in params.values())
    assert {c[0] for c in counts.values()} == {300, 513} and {c[1] for c in counts.values()} == {1, 3}
    assert counts["clones_only"][3] == 0 and counts["clones_only"][2] > counts["clones_only"][0] - 1
    assert counts["splits_only"][3] > 100 and counts["both"][3] > 100 and counts["nothing_over_thresh"][3] == 0
    assert counts["nothing_over_thresh"][2] < 300                                            # the closing prune still acts
    for name in ("accumulate_only", "accumulate_only_aniso", "after_stop"):
        assert counts[name][2] == counts[name][0] and z[name + "/normal_calls"] == 0
    with np.errstate(all="ignore"):
        assert np.isnan(z["denom_zero_rows/in/var/means2D_gradient_accum"] / z["denom_zero_rows/in/var/denom"]).sum() > 20


@pytest.mark.parametrize("name", F.densify_cases())
def test_densify_stepwise_restatement_matches_the_reference(name, monkeypatch):
    """tests/test_gpu_densify._densify_stepwise, the restatement the larger GPU cases are checked against, on the CPU under the reference's
    recorded draw: every row, Adam moment and accumulator bit for bit"""
    from test_gpu_densify import _densify_stepwise
    params, variables, opt, it, dd, draw, exp = F.densify_case(name)
    plain, mom = F.plain_state(params, opt)
    normal = F.RecordedNormal(draw)
    monkeypatch.setattr(torch, "normal", normal)
    var0 = {k: v for k, v in variables.items() if k != "means2D"}
    if it > dd["stop_after"]:                                                                # nothing happens any more, accumulation included
        got_p, got_m, got_v = plain, mom, var0
    else:
        got_p, got_m, got_v = _densify_stepwise(plain, mom, var0, it, dd, variables["means2D"].grad, variables["seen"])
    assert normal.calls == (draw is not None)
    for k in F.DKEYS:
        assert np.array_equal(got_p[k].numpy(), exp["param/" + k]), k
        assert np.array_equal(got_m[k][0].numpy(), exp["exp_avg/" + k]) and np.array_equal(got_m[k][1].numpy(), exp["exp_avg_sq/" + k]), k
    for k in F.DVARS + ("seen", "scene_radius"):
        assert np.array_equal(got_v[k].numpy(), exp["var/" + k]), k
    assert np.array_equal(exp["step"], np.full(8, 2.0))
    for k in ("cam_unnorm_rots", "cam_trans"):
        assert np.array_equal(params[k].detach().numpy(), exp["param/" + k])
