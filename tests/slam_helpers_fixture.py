"""Readers and comparisons for tests/golden/slam_helpers/*.npz (the reference's own outputs, written by
tests/golden/make_slam_helpers_golden.py), shared by the CPU and the GPU suites.  Nothing here touches a device."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "slam_helpers")
PARAM_KEYS = ("means3D", "unnorm_rotations", "logit_opacities", "log_scales", "cam_unnorm_rots", "cam_trans")
FWD_KEYS = ("means3D", "unnorm_rotations", "rotations", "opacities", "scales", "depth_sil")
EPS = 1e-12          # F.normalize's
EDGE_ROWS = 4        # rows 0..3 of the edge cases' unnorm_rotations have norm 0, 5e-20, 5e-13, 2e-12
ROT_PARAMS, ROT_TRANSFORMED = 0, 1

_cache = {}


def load(fname):
    if fname not in _cache:
        with np.load(os.path.join(GOLD, fname), allow_pickle=False) as z:
            _cache[fname] = {k: z[k] for k in z.files}
    return _cache[fname]


# ---------------------------------------------------------------- frame prep ----------------------------------------------------------------
def frame_prep_cases():
    return sorted(k[:-len("/meta")] for k in load("frame_prep.npz") if k.endswith("/meta"))


def frame_prep_case(name):
    """dict(builder, rot_source, inputs, P, S, time_idx, gaussians_grad, camera_grad, w2c | None, out, grads (None where the reference left
    .grad unset), upstream)"""
    from test_frame_prep import make_grads
    z = load("frame_prep.npz")
    builder, key = (str(s) for s in z[name + "/builder_inputs"])
    tidx, gg, cg = (int(v) for v in z[name + "/meta"])
    inputs = {k: z["%s/%s" % (key, k)] for k in PARAM_KEYS}
    P, S = inputs["means3D"].shape[0], inputs["log_scales"].shape[1]
    fwd_from = name if gg and cg else name[:name.index("_g")] + "_g1_c1"     # the detach flags change no value: one forward per family
    out = {k: z["%s/out/%s" % (fwd_from, k)] for k in FWD_KEYS + ("sil_color",) if "%s/out/%s" % (fwd_from, k) in z}
    none = dict(zip(PARAM_KEYS, (bool(v) for v in z[name + "/grad_is_none"])))
    grads = {k: (None if none[k] else z["%s/grad/%s" % (name, k)]) for k in PARAM_KEYS}
    return dict(name=name, builder=builder, rot_source=ROT_PARAMS if builder == "semantic" else ROT_TRANSFORMED, inputs=inputs, P=P, S=S,
                time_idx=tidx, gaussians_grad=bool(gg), camera_grad=bool(cg), w2c=z.get(name + "/w2c"), out=out, grads=grads,
                upstream=make_grads(P, builder == "depthsil"), edge=name.startswith("edge_"))


def assert_forward(name, got, want):
    """FWD_RTOL / FWD_ATOL of tests/test_gpu_frame_prep.py; NaN and +-inf have to sit where the reference has them"""
    from test_gpu_frame_prep import FWD_ATOL, FWD_RTOL
    np.testing.assert_allclose(np.asarray(got), want, rtol=FWD_RTOL, atol=FWD_ATOL, equal_nan=True, err_msg=name)


def forward_holds(got, want):
    from test_gpu_frame_prep import FWD_ATOL, FWD_RTOL
    return bool(np.allclose(np.asarray(got), want, rtol=FWD_RTOL, atol=FWD_ATOL, equal_nan=True))


def assert_gradient(name, got, want, rows=None):
    """BWD_TOL of tests/test_gpu_frame_prep.py, relative to the largest finite entry of the reference's tensor; classes (finite, +inf,
    -inf, NaN) must agree element for element.  rows: compare these rows one by one, each against its own largest entry."""
    from test_gpu_frame_prep import BWD_TOL
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if rows is not None:
        for r in rows:
            assert_gradient("%s row %d" % (name, r), got[r], want[r])
        return 0.0
    for cls in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(cls(got), cls(want)), "%s: %s sits elsewhere\n got %s\nwant %s" % (name, cls.__name__, got, want)
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    scale = max(np.abs(want[fin]).max(), 1e-30)
    err = np.abs(got[fin] - want[fin]).max() / scale
    assert err <= BWD_TOL, "%s: max err %.3g of scale %.3g" % (name, err, scale)
    return err


def expected_below_eps_rows(case):
    """what torch.autograd gives the quaternion rows with |u| < eps (rows 0, 1, 2) in the isotropic semantic builder, where
    rotations = F.normalize(params[u]) and the transformed quaternions are u itself: g_rotations / eps + g_unnorm_rotations"""
    assert case["S"] == 1 and case["builder"] == "semantic"
    up = case["upstream"]
    return up["rotations"][:3].astype(np.float64) / float(np.float32(EPS)) + up["unnorm_rotations"][:3]


def oracle_backward(O, case):
    """oracle/frame_prep_oracle.backward under the case's detach flags (slam_helpers.py:292-314): camera_grad = False leaves the pose
    without gradient, gaussians_grad = False leaves means3D without and the quaternions with only what the builder reads from params"""
    c = case
    kw = dict(time_idx=c["time_idx"], rot_source=c["rot_source"], w2c=c["w2c"])
    bo = O.backward(**c["inputs"], grads=c["upstream"], **kw)
    res = dict(means3D=bo["means3D"], unnorm_rotations=bo["unnorm_rotations"], logit_opacities=bo["logit_opacities"],
               log_scales=bo["log_scales"], cam_unnorm_rots=bo["cam_unnorm_rot"], cam_trans=bo["cam_tran"])
    if not c["gaussians_grad"]:
        res["means3D"] = None
        res["unnorm_rotations"] = None
        if c["rot_source"] == ROT_PARAMS:
            assert c["S"] == 1                                   # the fixture's flag cases: isotropic semantic, anisotropic rendervar
            only = dict(c["upstream"], unnorm_rotations=None, means3D=None)
            res["unnorm_rotations"] = O.backward(**c["inputs"], grads=only, **kw)["unnorm_rotations"]
    if not c["camera_grad"]:
        res["cam_unnorm_rots"] = res["cam_trans"] = None
    return res


def check_gradients(case, got, label=""):
    """got: dict over PARAM_KEYS of arrays or None; pose gradients either the column time_idx ([4] / [3]) or the whole [1,C,T] tensor, whose
    other columns must then be exactly zero.  Returns the largest relative error met."""
    worst = 0.0
    for k in PARAM_KEYS:
        want = case["grads"][k]
        assert (got[k] is None) == (want is None), "%s %s%s: gradient is %s, the reference's is %s" % (
            case["name"], k, label, "None" if got[k] is None else "set", "None" if want is None else "set")
        if want is None:
            continue
        g = np.asarray(got[k])
        if k.startswith("cam_"):
            other = np.delete(want[0], case["time_idx"], axis=1)
            assert not other.any(), "fixture: the reference's pose gradient has another column set"
            if g.ndim == 3:
                assert not np.delete(g[0], case["time_idx"], axis=1).any(), "%s %s: a column other than time_idx is not zero" % (case["name"], k)
                g = g[0, :, case["time_idx"]]
            want = want[0, :, case["time_idx"]]
        worst = max(worst, assert_gradient("%s %s%s" % (case["name"], k, label), g, want))
        if case["edge"] and k == "unnorm_rotations":
            assert_gradient("%s %s%s" % (case["name"], k, label), g, want, rows=range(EDGE_ROWS))
    return worst


# ------------------------------------------------------------------ densify -----------------------------------------------------------------
DKEYS = ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales", "semantic")
ALL_KEYS = DKEYS + ("cam_unnorm_rots", "cam_trans")
DD_KEYS = ("start_after", "remove_big_after", "stop_after", "densify_every", "grad_thresh", "num_to_split_into", "removal_opacity_threshold",
           "final_removal_opacity_threshold", "reset_opacities", "reset_opacities_every")
DVARS = ("means2D_gradient_accum", "denom", "max_2D_radius")


def densify_cases():
    return sorted(k[:-len("/state")] for k in load("densify_gradient.npz") if k.endswith("/state"))


def densify_case(name, device="cpu"):
    """(params as Parameters, variables, a torch.optim.Adam carrying the fixture's moments and steps, iter, densify_dict, recorded normal
    draw | None, expected outputs as arrays)"""
    z = load("densify_gradient.npz")
    state = str(z[name + "/state"])
    params = {k: torch.nn.Parameter(torch.tensor(z["%s/param/%s" % (state, k)]).to(device)) for k in ALL_KEYS}
    opt = torch.optim.Adam([{"params": [v], "name": k, "lr": 1e-2} for k, v in params.items()])
    for i, (k, v) in enumerate(params.items()):
        opt.state[v] = {"step": torch.tensor(float(z[state + "/step"][i])), "exp_avg": torch.tensor(z["%s/exp_avg/%s" % (state, k)]).to(device),
                        "exp_avg_sq": torch.tensor(z["%s/exp_avg_sq/%s" % (state, k)]).to(device)}
    variables = {k: torch.tensor(z["%s/in/var/%s" % (name, k)]).to(device) for k in DVARS + ("seen", "scene_radius")}
    m2d = torch.zeros(params["means3D"].shape[0], 3, device=device, requires_grad=True)
    m2d.grad = torch.tensor(z[name + "/in/means2D_grad"]).to(device)
    variables["means2D"] = m2d
    cfg = z[name + "/iter_and_densify_dict"]
    dd = dict(zip(DD_KEYS, (float(v) for v in cfg[1:])))
    for k in ("start_after", "remove_big_after", "stop_after", "densify_every", "num_to_split_into", "reset_opacities_every"):
        dd[k] = int(dd[k])
    dd["reset_opacities"] = bool(dd["reset_opacities"])
    draw = z.get(name + "/normal")
    assert int(z[name + "/normal_calls"]) == (draw is not None)
    exp = {k[len(name) + 5:]: v for k, v in z.items() if k.startswith(name + "/out/")}
    return params, variables, opt, int(cfg[0]), dd, draw, exp


class RecordedNormal:
    """stands in for torch.normal: hands out the reference's own draw, and fails if another shape is asked for"""

    def __init__(self, draw):
        self.draw, self.calls = draw, 0

    def __call__(self, mean=None, std=None, **kw):
        assert not kw and mean is not None and std is not None
        self.calls += 1
        assert self.draw is not None, "torch.normal was called; the reference did not call it"
        shape = tuple(torch.broadcast_shapes(mean.shape, std.shape))
        assert shape == tuple(self.draw.shape), "torch.normal asked for %s, the reference drew %s" % (shape, tuple(self.draw.shape))
        assert not mean.any()
        return torch.tensor(self.draw).to(device=std.device, dtype=std.dtype)


def plain_state(params, opt):
    plain = {k: params[k].detach().clone() for k in DKEYS}
    mom = {k: (opt.state[params[k]]["exp_avg"].clone(), opt.state[params[k]]["exp_avg_sq"].clone()) for k in DKEYS}
    return plain, mom
