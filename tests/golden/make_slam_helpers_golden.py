"""Generates tests/golden/slam_helpers/{frame_prep,camera,densify_gradient}.npz: inputs and outputs of the REFERENCE's own

    transform_to_frame, transformed_params2rendervar / 2silhouette / 2rendervar_semantic / 2depthplussilhouette   (utils/slam_helpers.py)
    setup_camera                                                                                                 (utils/recon_helpers.py)
    scale_intrinsics                                                                              (datasets/gradslam_datasets/datautils.py)
    densify                                                                                                      (utils/slam_external.py)

imported from /root/reference in the build container and run, unmodified, on CPU tensors.  Only data is stored (arrays and scalars, no
reference source).  Run by hand: python tests/golden/make_slam_helpers_golden.py  — never on a GPU machine, and no test imports this file.

How functions that say device="cuda" run without one: `PlaceOnCpu` below is a torch.overrides.TorchFunctionMode that rewrites a
device="cuda..." keyword argument to "cpu" and makes Tensor.cuda() return its tensor.  That changes where a tensor lives and nothing of the
arithmetic.  It also keeps a copy of every torch.normal result, so that a test can hand the same draw to the code under test.

utils/recon_helpers.py imports GaussianRasterizationSettings from diff_gaussian_rasterization; this repository's package needs its built
library to import, so a stand-in module with a NamedTuple of the same twelve field names (this repository's own list,
hier-slam_amd/diff_gaussian_rasterization/__init__.py) is registered first.  datautils.py is loaded by file path: its package's __init__
imports dataset loaders whose dependencies are not installed.

What the reference's functions turned out to do, recorded here because the fixtures carry it:
  * densify raises when `variables` holds 'timestep' (remove_points indexes it with the mask of the GROWN map): the key is left out.
  * densify with log_scales [P,3] draws torch.normal(mean [n,3], std [n,9]) and raises, whether or not a Gaussian is split; the
    three-column cases are therefore the ones in which densify never reaches that line (a non-densify iteration, iter > stop_after).
  * transformed_params2rendervar_semantic tiles log_scales [P,3] to scales [P,9]; the fixture keeps the first three columns (the
    repository's builder returns [P,3], see hsr_utils/slam_helpers.py) and the upstream gradient is put on those three.
Upstream gradients are tests/test_frame_prep.make_grads(P, with_sil) (seed 1), inputs tests/test_frame_prep.make_inputs(P, S, frames=6,
seed) — both restated here so that this file imports nothing of the suite; the tests rebuild the upstream gradients from make_grads and
read everything else from the fixture.
"""
import importlib.util
import io
import math
import os
import sys
import types
import zipfile
from typing import NamedTuple

import numpy as np
import torch
from torch.overrides import TorchFunctionMode

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "slam_helpers")
REF = "/root/reference"
sys.path.insert(0, REF)


class PlaceOnCpu(TorchFunctionMode):
    """placement only: device='cuda...' -> 'cpu', Tensor.cuda() -> the tensor itself; torch.normal results are recorded"""

    def __init__(self):
        super().__init__()
        self.normal_draws = []

    def __torch_function__(self, func, types_, args=(), kwargs=None):
        kwargs = dict(kwargs or {})
        if func is torch.Tensor.cuda:
            return args[0]
        if "device" in kwargs and kwargs["device"] is not None and str(kwargs["device"]).startswith("cuda"):
            kwargs["device"] = "cpu"
        out = func(*args, **kwargs)
        if func is torch.normal:
            self.normal_draws.append(out.detach().clone())
        return out


class GaussianRasterizationSettings(NamedTuple):     # this repository's own field list
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def import_reference():
    stand_in = types.ModuleType("diff_gaussian_rasterization")
    stand_in.GaussianRasterizationSettings = GaussianRasterizationSettings
    sys.modules["diff_gaussian_rasterization"] = stand_in
    from utils import recon_helpers, slam_external, slam_helpers
    spec = importlib.util.spec_from_file_location("ref_datautils", os.path.join(REF, "datasets", "gradslam_datasets", "datautils.py"))
    datautils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(datautils)
    return slam_helpers, slam_external, recon_helpers, datautils


# ------------------------------------------------------------------ frame prep ------------------------------------------------------------------
FRAMES = 6
PARAM_KEYS = ("means3D", "unnorm_rotations", "logit_opacities", "log_scales", "cam_unnorm_rots", "cam_trans")


def make_inputs(P, S, frames=FRAMES, seed=0):      # = tests/test_frame_prep.make_inputs
    g = np.random.default_rng(seed)
    return dict(means3D=g.normal(0, 2, (P, 3)).astype(np.float32), unnorm_rotations=g.normal(0, 1, (P, 4)).astype(np.float32),
                logit_opacities=g.normal(0, 1.5, (P, 1)).astype(np.float32), log_scales=g.normal(-4, 0.5, (P, S)).astype(np.float32),
                cam_unnorm_rots=(g.normal(0, 1, (1, 4, frames)) * 1.7).astype(np.float32),
                cam_trans=g.normal(0, 0.5, (1, 3, frames)).astype(np.float32))


def make_grads(P, with_sil, seed=1):                # = tests/test_frame_prep.make_grads
    g = np.random.default_rng(seed)
    d = dict(means3D=g.normal(0, 1, (P, 3)), unnorm_rotations=g.normal(0, 1, (P, 4)), rotations=g.normal(0, 1, (P, 4)),
             opacities=g.normal(0, 1, (P, 1)), scales=g.normal(0, 1, (P, 3)))
    if with_sil:
        d["depth_sil"] = g.normal(0, 1, (P, 3))
    return {k: v.astype(np.float32) for k, v in d.items()}


def quat_to_matrix(q):
    r, x, y, z = np.asarray(q, np.float32) / np.float32(np.sqrt(np.sum(np.asarray(q, np.float32) ** 2, dtype=np.float32)))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                     [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                     [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]], np.float32)


def depthsil_w2c():
    """the tilted world-to-camera matrix of tests/test_frame_prep.py (quaternion (0.9, 0.1, -0.3, 0.2), translation (0.1, -0.2, 0.3))"""
    w2c = np.eye(4, dtype=np.float32)
    w2c[:3, :3] = quat_to_matrix([0.9, 0.1, -0.3, 0.2])
    w2c[:3, 3] = (0.1, -0.2, 0.3)
    return w2c


def edge_inputs(S, pose_edge=False):
    """P = 64: quaternion rows 0..3 of norm 0, 5e-20, 5e-13 and 2e-12 (F.normalize's eps is 1e-12), logit_opacities of +-90 (exp(-x)
    overflows fp32 / the sigmoid saturates), log_scales of -90 and 40.  pose_edge: the pose column time_idx = 2 has norm 5e-13."""
    inp = make_inputs(64, S, seed=7)
    u = inp["unnorm_rotations"]
    u[0] = 0.0
    u[1] = np.array([3e-20, -4e-20, 0.0, 0.0], np.float32)
    u[2] = np.array([3e-13, -4e-13, 0.0, 0.0], np.float32)
    u[3] = np.array([0.0, 1.2e-12, 0.0, -1.6e-12], np.float32)
    inp["logit_opacities"][4, 0], inp["logit_opacities"][5, 0] = 90.0, -90.0
    inp["log_scales"][6, 0], inp["log_scales"][7, S - 1] = -90.0, 40.0
    if pose_edge:
        inp["cam_unnorm_rots"][0, :, 2] = np.array([3e-13, 0.0, 0.0, -4e-13], np.float32)
    return inp


def frame_prep_case(SH, out, name, inp, builder, tidx, gaussians_grad=True, camera_grad=True):
    P = inp["means3D"].shape[0]
    with_sil = builder == "depthsil"
    t = {k: torch.tensor(v, requires_grad=True) for k, v in inp.items()}
    t["rgb_colors"], t["semantic"] = torch.zeros(P, 3), torch.zeros(P, 5)    # handed through untouched: not part of the fixture
    w2c = depthsil_w2c() if with_sil else None
    with PlaceOnCpu():
        tg = SH.transform_to_frame(t, tidx, gaussians_grad=gaussians_grad, camera_grad=camera_grad)
        if builder == "semantic":
            rv = SH.transformed_params2rendervar_semantic(t, tg)
        elif builder == "rendervar":
            rv = SH.transformed_params2rendervar(t, tg)
        elif builder == "silhouette":
            rv = SH.transformed_params2silhouette(t, tg)
        else:
            rv = SH.transformed_params2depthplussilhouette(t, torch.tensor(w2c), tg)
        scales = rv["scales"][:, :3]                                   # [P,9] from the semantic builder with S = 3: see the docstring
        up = {k: torch.tensor(v) for k, v in make_grads(P, with_sil).items()}
        loss = (rv["means3D"] * up["means3D"]).sum() + (tg["unnorm_rotations"] * up["unnorm_rotations"]).sum() \
            + (rv["rotations"] * up["rotations"]).sum() + (rv["opacities"] * up["opacities"]).sum() + (scales * up["scales"]).sum()
        if with_sil:
            loss = loss + (rv["colors_precomp"] * up["depth_sil"]).sum()
        loss.backward()
    out[name + "/meta"] = np.asarray([tidx, int(bool(gaussians_grad)), int(bool(camera_grad))])   # few, packed arrays: a member costs ~250 B
    if w2c is not None:
        out[name + "/w2c"] = w2c
    fwd = dict(means3D=rv["means3D"], unnorm_rotations=tg["unnorm_rotations"], rotations=rv["rotations"], opacities=rv["opacities"],
               scales=scales)
    if with_sil:
        fwd["depth_sil"] = rv["colors_precomp"]
    if builder == "silhouette":
        fwd["sil_color"] = rv["colors_precomp"]
    if gaussians_grad and camera_grad:               # the flags detach, they do not change a value: flags_*_g1_c1 holds the forward
        for k, v in fwd.items():
            out["%s/out/%s" % (name, k)] = v.detach().numpy().copy()
    assert tuple(rv["means2D"].shape) == (P, 3) and not rv["means2D"].detach().any()
    out[name + "/grad_is_none"] = np.asarray([t[k].grad is None for k in PARAM_KEYS])             # in PARAM_KEYS order
    for k in PARAM_KEYS:
        if t[k].grad is not None:
            out["%s/grad/%s" % (name, k)] = t[k].grad.numpy().copy()


def make_frame_prep(SH):
    out = {}
    inputs = {}

    def shared(P, S):
        key = "inputs/P%d_S%d" % (P, S)
        if key not in inputs:
            inputs[key] = make_inputs(P, S, seed=P + S)
            for k, v in inputs[key].items():
                out["%s/%s" % (key, k)] = v
        return key, inputs[key]

    def add(name, P, S, builder, tidx, **flags):
        key, inp = shared(P, S)
        out[name + "/builder_inputs"] = np.asarray([builder, key])
        frame_prep_case(SH, out, name, inp, builder, tidx, **flags)

    builders = ("rendervar", "semantic", "silhouette", "depthsil")
    for i, b in enumerate(builders):                                    # P = 1: every builder and S
        for S in (1, 3):
            tidx = (FRAMES - 1, 0)[(i + S // 3) % 2]
            add("p1_%s_S%d_t%d" % (b, S, tidx), 1, S, b, tidx)
    for i, b in enumerate(builders):                                    # P = 257 (one forward block + 1): every builder and S
        for S in (1, 3):
            tidx = (0, FRAMES - 1)[(i + S // 3) % 2]
            add("p257_%s_S%d_t%d" % (b, S, tidx), 257, S, b, tidx)
    add("p1025_semantic_S1_t5", 1025, 1, "semantic", FRAMES - 1)         # P = 1025 (one 4 x 256 backward block + 1)
    add("p1025_depthsil_S3_t0", 1025, 3, "depthsil", 0)
    for b, S in (("semantic", 1), ("rendervar", 3)):                    # the detach flags of transform_to_frame
        for gg in (True, False):
            for cg in (True, False):
                add("flags_%s_S%d_g%d_c%d" % (b, S, gg, cg), 257, S, b, 2, gaussians_grad=gg, camera_grad=cg)
    for S, b in ((3, "rendervar"), (1, "semantic"), (3, "semantic"), (1, "depthsil")):   # the edge rows
        name = "edge_%s_S%d" % (b, S)
        inp = edge_inputs(S)
        for k, v in inp.items():
            out["inputs/%s/%s" % (name, k)] = v
        out[name + "/builder_inputs"] = np.asarray([b, "inputs/" + name])
        frame_prep_case(SH, out, name, inp, b, 2)
    for S, b in ((3, "rendervar"), (1, "semantic")):                    # ... and the same clamp on the pose quaternion
        name = "edge_pose_%s_S%d" % (b, S)
        inp = edge_inputs(S, pose_edge=True)
        for k, v in inp.items():
            out["inputs/%s/%s" % (name, k)] = v
        out[name + "/builder_inputs"] = np.asarray([b, "inputs/" + name])
        frame_prep_case(SH, out, name, inp, b, 2)
    return out


# ------------------------------------------------------------------- camera ---------------------------------------------------------------------
def tilted_w2c(angle, t):                            # = tests/scenes.tilted_w2c
    w2c = np.eye(4)
    w2c[:3, :3] = np.array([[math.cos(angle), 0, math.sin(angle)], [0, 1, 0], [-math.sin(angle), 0, math.cos(angle)]])
    w2c[:3, 3] = t
    return w2c


def make_camera(RH, DU):
    out = {}
    W, H = 96, 64
    cases = [("replica_identity", 1200, 680, np.array([[600.0, 0, 599.5], [0, 600.0, 339.5], [0, 0, 1]]), np.eye(4), 0.01, 100),
             ("off_centre_tilted", W, H, np.array([[0.97 * W, 0.0, 0.41 * W], [0.0, 1.07 * W, 0.57 * H], [0.0, 0.0, 1.0]]),
              tilted_w2c(0.15, (0.05, 0.1, 0.1)), 0.01, 100),
             ("one_by_one", 1, 1, np.array([[0.8, 0, 0.5], [0, 0.9, 0.5], [0, 0, 1]]), tilted_w2c(0.2, (0.1, -0.05, 0.2)), 0.01, 100),
             ("near_far", 160, 120, np.array([[150.0, 0, 79.5], [0, 150.0, 59.5], [0, 0, 1]]), tilted_w2c(-0.4, (0.3, 0.0, -0.1)), 0.25, 17.5)]
    for name, w, h, k, w2c, near, far in cases:
        with PlaceOnCpu():
            cam = RH.setup_camera(w, h, k, w2c, near=near, far=far)
        for key, v in (("w", w), ("h", h), ("k", k), ("w2c", w2c), ("near", near), ("far", far)):
            out["setup/%s/in/%s" % (name, key)] = np.asarray(v)
        for key in ("viewmatrix", "projmatrix", "campos", "bg"):
            out["setup/%s/out/%s" % (name, key)] = getattr(cam, key).numpy().copy()
        for key in ("tanfovx", "tanfovy", "image_height", "image_width", "scale_modifier", "sh_degree", "prefiltered", "debug"):
            out["setup/%s/out/%s" % (name, key)] = np.asarray(getattr(cam, key))
    g = np.random.default_rng(3)
    k3 = np.array([[600.0, 0, 599.5], [0, 600.0, 339.5], [0, 0, 1]])
    k4 = np.eye(4); k4[:3, :3] = k3 * np.array([[1.013, 1, 0.987], [1, 0.991, 1.021], [1, 1, 1]])
    kb = np.stack([k3, k3 * np.array([[0.5, 1, 0.25], [1, 0.75, 1.5], [1, 1, 1]])]) + np.array([[g.random() * 1e-3, 0, 0], [0, 0, 0], [0, 0, 0]])
    for name, arr in (("numpy_3x3_f64", k3), ("tensor_4x4_f32", torch.tensor(k4, dtype=torch.float32)),
                      ("tensor_batched_2x3x3_f64", torch.tensor(kb, dtype=torch.float64))):
        for rname, hr, wr in (("half", 0.5, 0.5), ("64_96", 64 / 680, 96 / 1200)):
            before = (arr.numpy() if torch.is_tensor(arr) else arr).copy()
            got = DU.scale_intrinsics(arr, hr, wr)
            assert np.array_equal(np.asarray(arr), before)
            key = "scale/%s/%s" % (name, rname)
            out[key + "/in"] = before
            out[key + "/h_ratio"], out[key + "/w_ratio"] = np.asarray(hr), np.asarray(wr)
            out[key + "/out"] = np.asarray(got).copy()
            out[key + "/out_is_tensor"] = np.asarray(torch.is_tensor(got))
    return out


# ----------------------------------------------------------- gradient-driven densify ------------------------------------------------------------
DKEYS = ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales", "semantic")
DCOLS = dict(means3D=3, rgb_colors=3, unnorm_rotations=4, logit_opacities=1, log_scales=1, semantic=1)
DENSIFY_DICT = dict(start_after=100, remove_big_after=300, stop_after=500, densify_every=100, grad_thresh=6e-4, num_to_split_into=2,
                    removal_opacity_threshold=0.3, final_removal_opacity_threshold=0.5, reset_opacities=False, reset_opacities_every=250)


def densify_state(P, seed, scales_cols):
    """as make_densify_golden.make_state: a torch.optim.Adam whose exp_avg / exp_avg_sq / step come from two real steps"""
    g = torch.Generator().manual_seed(seed)
    cols = dict(DCOLS, log_scales=scales_cols)
    params = {k: torch.nn.Parameter(torch.randn(P, cols[k], generator=g)) for k in DKEYS}
    with torch.no_grad():
        params["logit_opacities"].mul_(3.0)
        params["log_scales"].mul_(0.7).sub_(2.0)
    params["cam_unnorm_rots"] = torch.nn.Parameter(torch.randn(1, 4, 5, generator=g))
    params["cam_trans"] = torch.nn.Parameter(torch.randn(1, 3, 5, generator=g))
    opt = torch.optim.Adam([{"params": [v], "name": k, "lr": 1e-2} for k, v in params.items()])
    for _ in range(2):
        opt.zero_grad()
        sum((v * torch.randn(v.shape, generator=g)).sum() for v in params.values()).backward()
        opt.step()
    opt.zero_grad()
    extent = torch.exp(params["log_scales"].detach()).max(dim=1).values
    return params, None, opt, None, extent


def dump_state(prefix, params, variables, opt, out):
    steps = []
    for k, v in params.items():
        out["%s/param/%s" % (prefix, k)] = v.detach().numpy().copy()
        st = opt.state[[g for g in opt.param_groups if g["name"] == k][0]["params"][0]]
        out["%s/exp_avg/%s" % (prefix, k)] = st["exp_avg"].numpy().copy()
        out["%s/exp_avg_sq/%s" % (prefix, k)] = st["exp_avg_sq"].numpy().copy()
        steps.append(float(st["step"]))
    if params:
        out[prefix + "/step"] = np.asarray(steps)                      # in the order of DKEYS + the two pose tensors
    for k, v in variables.items():
        if k != "means2D":
            out["%s/var/%s" % (prefix, k)] = v.numpy().copy()


def make_densify(SE):
    out = {}
    # (case, P, log_scales columns, iter, scene radius as a multiple of extent quantile q [q, multiple], densify_dict overrides)
    # the multiple is never 1: with an odd P the median IS a Gaussian's extent, and its small / large decision would hang on one rounding
    cases = [("clones_only", 300, 1, 200, (1.0, 2.0), {}),
             ("splits_only", 300, 1, 200, (0.0, 0.5), dict(remove_big_after=10 ** 6)),
             ("both", 513, 1, 300, (0.5, 1.003), {}),
             ("both_final_threshold", 300, 1, 500, (0.5, 1.003), {}),
             ("before_remove_big", 300, 1, 100, (0.5, 1.003), {}),
             ("nothing_over_thresh", 300, 1, 300, (0.5, 1.003), dict(grad_thresh=1e9)),
             ("denom_zero_rows", 300, 1, 200, (0.5, 1.003), {}),
             ("accumulate_only", 300, 1, 150, (0.5, 1.003), {}),
             ("accumulate_only_aniso", 300, 3, 150, (0.5, 1.003), {}),
             ("reset_opacities", 300, 1, 200, (0.5, 1.003), dict(reset_opacities=True, reset_opacities_every=200)),
             ("after_stop", 300, 1, 700, (0.5, 1.003), {})]
    for name, P, sc, it, (q, mult), over in cases:
        params, variables, opt, grad2d, extent = densify_state(P, seed=10 * P + sc, scales_cols=sc)   # one map per (P, columns)
        state = "state/P%d_S%d" % (P, sc)
        if state + "/param/means3D" not in out:
            dump_state(state, params, {}, opt, out)
        out[name + "/state"] = np.asarray(state)
        g = torch.Generator().manual_seed(len(name) * 1000 + P)           # ... bookkeeping vectors of its own per case
        variables = dict(means2D_gradient_accum=torch.rand(P, generator=g) * 2e-3, denom=torch.randint(0, 4, (P,), generator=g).float(),
                         max_2D_radius=torch.rand(P, generator=g) * 9, seen=torch.rand(P, generator=g) < 0.6)
        grad2d = torch.randn(P, 3, generator=g) * 1e-3
        if name == "nothing_over_thresh":
            variables["denom"].clamp_(min=1.0)                            # no x / 0 = inf, which is over any threshold
        variables["scene_radius"] = torch.tensor(float(torch.quantile(extent, q)) / 0.01 * mult)
        if name == "denom_zero_rows":   # rows nobody has seen: 0 / 0 = NaN -> 0 on the even ones, x / 0 = inf (over any threshold) on the odd ones
            idx = torch.arange(P)
            unseen = idx % 3 == 0
            variables["seen"][unseen] = False
            variables["denom"][unseen] = 0.0
            variables["means2D_gradient_accum"][unseen & (idx % 2 == 0)] = 0.0
        dd = dict(DENSIFY_DICT, **over)
        m2d = torch.zeros(P, 3, requires_grad=True)
        m2d.grad = grad2d.clone()
        variables["means2D"] = m2d
        dump_state(name + "/in", {}, variables, opt, out)
        out[name + "/in/means2D_grad"] = grad2d.numpy().copy()
        out[name + "/iter_and_densify_dict"] = np.asarray([float(it)] + [float(dd[k]) for k in DENSIFY_DICT])   # in DENSIFY_DICT's order
        torch.manual_seed(4321)
        with PlaceOnCpu() as mode:
            params, variables = SE.densify(params, variables, opt, it, dd)
        assert len(mode.normal_draws) <= 1
        out[name + "/normal_calls"] = np.asarray(len(mode.normal_draws))
        if mode.normal_draws:
            out[name + "/normal"] = mode.normal_draws[0].numpy().copy()
        dump_state(name + "/out", params, variables, opt, out)
        print("  %-24s P %d -> %d   normal draw %s" % (name, P, params["means3D"].shape[0],
                                                      tuple(mode.normal_draws[0].shape) if mode.normal_draws else None))
    return out


def save_npz(path, data):
    """np.savez_compressed with a fixed member date, so that a rerun gives the same bytes (numpy stamps each member with the clock)"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key, value in data.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def main():
    torch.set_num_threads(1)                                            # reductions in a fixed order: the files regenerate byte for byte
    SH, SE, RH, DU = import_reference()
    os.makedirs(OUT, exist_ok=True)
    for fname, data in (("frame_prep.npz", make_frame_prep(SH)), ("camera.npz", make_camera(RH, DU)),
                        ("densify_gradient.npz", make_densify(SE))):
        path = os.path.join(OUT, fname)
        save_npz(path, data)
        print("wrote %s: %d arrays, %d bytes" % (fname, len(data), os.path.getsize(path)))


if __name__ == "__main__":
    main()
