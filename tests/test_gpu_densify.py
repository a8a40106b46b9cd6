"""GPU parity for the densification step (include/hsr_densify.h) against oracle/densify_oracle.py, and the reference-named
add_new_gaussians_semantic on a small map."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("H,W,seed", [(48, 64, 0), (37, 53, 1), (680, 1200, 2), (16, 16, 3)])
def test_non_presence_points_match_oracle(H, W, seed):
    import densify_oracle as DO
    from hsr_utils import densify as D
    from test_densify import make_frame
    sil, rd, gt, col, K, w2c = make_frame(H, W, seed)
    t = lambda a: torch.tensor(a, device="cuda")
    pt_cld, msd, mask, ls = D.non_presence_points(t(sil), t(rd), t(gt), t(col), torch.tensor(K), t(w2c), 0.5)
    c2w = torch.inverse(torch.tensor(w2c)).numpy()
    o = DO.non_presence_points(sil, rd, gt, col, K, c2w, 0.5)
    assert np.array_equal(mask.cpu().numpy(), o["mask"])                      # integer decisions: bit-exact (incl. the median)
    assert pt_cld.shape[0] == int(o["mask"].sum())
    np.testing.assert_allclose(pt_cld[:, :3].cpu().numpy(), o["means3D"], rtol=1e-6, atol=1e-6)
    np.testing.assert_array_equal(pt_cld[:, 3:].cpu().numpy(), o["rgb"])      # order-preserving compaction
    np.testing.assert_allclose(msd.cpu().numpy(), o["mean3_sq_dist"], rtol=1e-6)
    np.testing.assert_allclose(ls[:, 0].cpu().numpy(), o["log_scales"], rtol=1e-5, atol=1e-6)


def test_no_new_points_and_bad_input():
    from hsr_utils import densify as D
    from test_densify import make_frame
    sil, rd, gt, col, K, w2c = make_frame(32, 40, 5, hole=False)
    t = lambda a: torch.tensor(a, device="cuda")
    pt_cld, msd, mask, ls = D.non_presence_points(t(sil), t(gt), t(gt), t(col), torch.tensor(K), t(w2c), 0.5)
    assert pt_cld.shape == (0, 6) and not mask.any()
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.non_presence_points(torch.tensor(sil), t(gt), t(gt), t(col), torch.tensor(K), t(w2c), 0.5)


def test_add_new_gaussians_semantic_grows_the_map_where_nothing_was_rendered():
    from hsr_utils import densify as D, setup_camera, make_scene
    W, H, K, P = 160, 120, 6, 3000
    kmat = np.array([[150.0, 0, 79.5], [0, 150.0, 59.5], [0, 0, 1]])
    cam = setup_camera(W, H, kmat, np.eye(4), device="cuda")
    sc = make_scene(P, W, H, K, kmat, seed=4, scale_mult=3.0)
    keep = sc["means3D"][:, 0] < 0                                            # a map that only covers the left half
    params = {"means3D": sc["means3D"][keep], "unnorm_rotations": sc["rotations"][keep],
              "logit_opacities": torch.full((int(keep.sum()), 1), 4.0), "log_scales": sc["scales"][keep][:, :1].log(),
              "rgb_colors": sc["colors_precomp"][keep], "semantic": sc["semantics_precomp"][keep]}
    params = {k: torch.nn.Parameter(v.clone().cuda()) for k, v in params.items()}
    params["cam_unnorm_rots"] = torch.nn.Parameter(torch.tensor([1.0, 0, 0, 0]).view(1, 4, 1).repeat(1, 1, 2).cuda())
    params["cam_trans"] = torch.nn.Parameter(torch.zeros(1, 3, 2).cuda())
    n0 = params["means3D"].shape[0]
    variables = {"timestep": torch.zeros(n0, device="cuda")}
    curr = {"cam": cam, "w2c": torch.eye(4, device="cuda"), "depth": torch.full((1, H, W), 2.0, device="cuda"),
            "im": torch.rand(3, H, W, device="cuda"), "intrinsics": torch.tensor(kmat, dtype=torch.float32)}
    params, variables = D.add_new_gaussians_semantic(params, variables, curr, 0.5, 1, "projective", K)
    n1 = params["means3D"].shape[0]
    added = params["means3D"][n0:]
    assert n1 > n0 and variables["timestep"].shape[0] == n1 and (variables["timestep"][n0:] == 1).all()
    assert float((added[:, 0] > -0.1).float().mean()) > 0.9                   # new points fill the uncovered right half
    np.testing.assert_allclose(added[:, 2].detach().cpu().numpy(), 2.0, rtol=1e-5)   # at the measured depth
    for k in ("rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales", "semantic"):
        assert params[k].shape[0] == n1 and isinstance(params[k], torch.nn.Parameter) and params[k].requires_grad
    assert variables["means2D_gradient_accum"].shape == (n1,) and variables["denom"].shape == (n1,)


def _half_map(W, H, K, P, semantic=True, scales_cols=1):
    from hsr_utils import setup_camera, make_scene
    kmat = np.array([[150.0, 0, 79.5], [0, 150.0, 59.5], [0, 0, 1]])
    cam = setup_camera(W, H, kmat, np.eye(4), device="cuda")
    sc = make_scene(P, W, H, K, kmat, seed=4, scale_mult=3.0)
    keep = sc["means3D"][:, 0] < 0                                            # a map that only covers the left half
    params = {"means3D": sc["means3D"][keep], "unnorm_rotations": sc["rotations"][keep],
              "logit_opacities": torch.full((int(keep.sum()), 1), 4.0), "log_scales": sc["scales"][keep][:, :scales_cols].log(),
              "rgb_colors": sc["colors_precomp"][keep]}
    if semantic:
        params["semantic"] = sc["semantics_precomp"][keep]
    params = {k: torch.nn.Parameter(v.clone().cuda()) for k, v in params.items()}
    params["cam_unnorm_rots"] = torch.nn.Parameter(torch.tensor([1.0, 0, 0, 0]).view(1, 4, 1).repeat(1, 1, 2).cuda())
    params["cam_trans"] = torch.nn.Parameter(torch.zeros(1, 3, 2).cuda())
    n0 = params["means3D"].shape[0]
    variables = {"timestep": torch.zeros(n0, device="cuda")}
    curr = {"cam": cam, "w2c": torch.eye(4, device="cuda"), "depth": torch.full((1, H, W), 2.0, device="cuda"),
            "im": torch.rand(3, H, W, device="cuda"), "intrinsics": torch.tensor(kmat, dtype=torch.float32)}
    return params, variables, curr, n0


def _torch_mask(final_opacity, rendered_depth, gt_depth, sil_thres):
    """scripts/hierslam.py:1317-1329 / :1225-1236 + :1248-1249 / :1337-1338 with torch CPU ops"""
    sil, rd, gt = final_opacity.cpu(), rendered_depth.cpu(), gt_depth.cpu()
    depth_error = torch.abs(gt - rd) * (gt > 0)
    m = (sil < sil_thres) | ((rd > gt) * (depth_error > 50 * depth_error.median()))
    return (m.reshape(-1) & (gt > 0).reshape(-1)).numpy()


@pytest.mark.parametrize("variant", ["semantic_newrender", "newtest_isotropic", "newtest_anisotropic"])
def test_the_densify_functions_the_mapping_loop_calls(variant):
    """add_new_gaussians_semantic_newrender (scripts/hierslam.py:1307-1352, called :1949) and add_new_gaussians_newtest
    (:1214-1262, called :1945): the silhouette is the FINAL OPACITY of one no-grad render with the semantic / plain
    rasterizer.  The selected pixels must equal the reference's mask expressions evaluated with torch CPU ops on the same
    rendered maps — bit for bit — and the map must grow by exactly those pixels, in row-major order."""
    from diff_gaussian_rasterization import GaussianRasterizer, GaussianRasterizer_semantic
    from hsr_utils import densify as D, slam_helpers as SH
    W, H, K, P = 160, 120, 6, 3000
    semantic = variant == "semantic_newrender"
    params, variables, curr, n0 = _half_map(W, H, K, P, semantic=semantic, scales_cols=3 if variant.endswith("anisotropic") else 1)
    curr["depth"][0, :10] = 0.0                                               # invalid depth rows are never densified
    tg = SH.transform_to_frame(params, 1, gaussians_grad=False, camera_grad=False)
    with torch.no_grad():
        if semantic:
            outs = GaussianRasterizer_semantic(curr["cam"])(**SH.transformed_params2rendervar_semantic(params, tg))
            depth, final_opacity = outs[3], outs[5]
        else:
            outs = GaussianRasterizer(curr["cam"])(**SH.transformed_params2rendervar(params, tg))
            depth, final_opacity = outs[2], outs[4]
    expect = _torch_mask(final_opacity[0], depth[0], curr["depth"][0], 0.5)
    if semantic:
        params, variables = D.add_new_gaussians_semantic_newrender(params, variables, curr, 0.5, 1, "projective", K)
    else:
        dist = "anisotropic" if variant.endswith("anisotropic") else "isotropic"
        params, variables = D.add_new_gaussians_newtest(params, variables, curr, 0.5, 1, "projective", dist)
    n1 = params["means3D"].shape[0]
    assert 0 < expect.sum() < expect.size and n1 - n0 == int(expect.sum())
    # the new points ARE the back-projection of the selected pixels, in row-major order (get_pointcloud, :144-194)
    ys, xs = np.nonzero(expect.reshape(H, W))
    z = curr["depth"][0].cpu().numpy()[ys, xs]
    exp_xyz = np.stack([(xs - 79.5) / 150.0 * z, (ys - 59.5) / 150.0 * z, z], 1)
    np.testing.assert_allclose(params["means3D"][n0:].detach().cpu().numpy(), exp_xyz, rtol=1e-5, atol=1e-6)
    exp_rgb = curr["im"].permute(1, 2, 0).reshape(-1, 3).cpu().numpy()[expect]
    np.testing.assert_array_equal(params["rgb_colors"][n0:].detach().cpu().numpy(), exp_rgb)
    exp_ls = np.log(np.sqrt((z / 150.0) ** 2))
    got_ls = params["log_scales"][n0:].detach().cpu().numpy()
    assert got_ls.shape == (n1 - n0, 3 if variant.endswith("anisotropic") else 1)
    np.testing.assert_allclose(got_ls, np.repeat(exp_ls[:, None], got_ls.shape[1], 1), rtol=1e-5, atol=1e-6)
    assert (variables["timestep"][n0:] == 1).all() and variables["denom"].shape == (n1,)
    assert ("semantic" in params) == semantic and (not semantic or params["semantic"].shape == (n1, K))
    with pytest.raises(ValueError):
        D.add_new_gaussians_newtest(params, variables, curr, 0.5, 1, "projective", "isotropic", flag_use_render=2)


# ---- prune / concat: pinned by the REFERENCE's own outputs (tests/golden/densify_prune_concat.npz, generated by
# tests/golden/make_densify_golden.py from utils/slam_external.py's prune_gaussians and cat_params_to_optimizer) ------------
GOLD = os.path.join(ROOT, "tests", "golden", "densify_prune_concat.npz")
KEYS = ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales", "semantic")


def _load_state(z, prefix):
    """params (cuda Parameters), variables, Adam optimizer whose state is the fixture's"""
    params = {k: torch.nn.Parameter(torch.tensor(z["%s/param/%s" % (prefix, k)]).cuda()) for k in KEYS + ("cam_unnorm_rots", "cam_trans")}
    opt = torch.optim.Adam([{"params": [v], "name": k, "lr": 1e-2} for k, v in params.items()])
    for k, v in params.items():
        if "%s/exp_avg/%s" % (prefix, k) in z:
            opt.state[v] = {"step": torch.tensor(float(z["%s/step/%s" % (prefix, k)])),
                            "exp_avg": torch.tensor(z["%s/exp_avg/%s" % (prefix, k)]).cuda(),
                            "exp_avg_sq": torch.tensor(z["%s/exp_avg_sq/%s" % (prefix, k)]).cuda()}
    variables = {k.split("/")[-1]: torch.tensor(z[k]).cuda() for k in z.files if k.startswith(prefix + "/var/")}
    return params, variables, opt


def _assert_state_equals(z, prefix, params, variables, opt):
    for k in KEYS + ("cam_unnorm_rots", "cam_trans"):
        exp = z["%s/param/%s" % (prefix, k)]
        assert isinstance(params[k], torch.nn.Parameter) and params[k].requires_grad
        assert np.array_equal(params[k].detach().cpu().numpy(), exp), k             # rows in order, bit for bit
        group = [g for g in opt.param_groups if g["name"] == k][0]
        assert group["params"][0] is params[k]
        st = opt.state.get(params[k], None)
        if "%s/exp_avg/%s" % (prefix, k) in z:
            assert np.array_equal(st["exp_avg"].cpu().numpy(), z["%s/exp_avg/%s" % (prefix, k)]), k
            assert np.array_equal(st["exp_avg_sq"].cpu().numpy(), z["%s/exp_avg_sq/%s" % (prefix, k)]), k
            assert float(st["step"]) == float(z["%s/step/%s" % (prefix, k)])
        else:
            assert not st
    for k in z.files:
        if k.startswith(prefix + "/var/"):
            assert np.array_equal(variables[k.split("/")[-1]].cpu().numpy(), z[k]), k
    assert len(opt.state) == sum(1 for k in params if "%s/exp_avg/%s" % (prefix, k) in z)   # no orphaned state entries


@pytest.mark.parametrize("case", ["prune_iter0", "prune_final_aniso", "prune_no_big", "prune_not_this_iter", "prune_reset_opacities"])
def test_prune_gaussians_matches_the_reference_outputs(case):
    from hsr_utils import slam_external as SE
    z = np.load(GOLD, allow_pickle=False)
    params, variables, opt = _load_state(z, case + "/in")
    pd = {k.split("/")[-1]: float(z[k]) for k in z.files if k.startswith(case + "/prune_dict/")}
    pd["reset_opacities"] = bool(pd["reset_opacities"])
    n_in = params["means3D"].shape[0]
    params, variables = SE.prune_gaussians(params, variables, opt, int(z[case + "/iter"]), pd)
    _assert_state_equals(z, case + "/out", params, variables, opt)
    n_out = z[case + "/out/param/means3D"].shape[0]
    assert (n_out < n_in) == (case not in ("prune_not_this_iter",))
    # the pruned map still trains: one more Adam step through the re-keyed state
    (params["means3D"].sum() + params["semantic"].sum()).backward()
    opt.step()


@pytest.mark.parametrize("case", ["cat_small", "cat_empty_map", "cat_nothing_new"])
def test_cat_params_to_optimizer_matches_the_reference_outputs(case):
    from hsr_utils import slam_external as SE
    z = np.load(GOLD, allow_pickle=False)
    params, variables, opt = _load_state(z, case + "/in")
    new = {k: torch.tensor(z["%s/new/%s" % (case, k)]).cuda() for k in KEYS}
    params = SE.cat_params_to_optimizer(new, params, opt)
    _assert_state_equals(z, case + "/out", params, {}, opt)


def test_remove_points_with_a_caller_mask_and_bad_input():
    from hsr_utils import slam_external as SE
    z = np.load(GOLD, allow_pickle=False)
    params, variables, opt = _load_state(z, "prune_iter0/in")
    P = params["means3D"].shape[0]
    g = torch.Generator().manual_seed(5)
    to_remove = (torch.rand(P, generator=g) < 0.37).cuda()
    exp = {k: params[k].detach()[~to_remove].cpu().numpy() for k in KEYS}
    exp_m = {k: opt.state[params[k]]["exp_avg"][~to_remove].cpu().numpy() for k in KEYS}
    exp_v = {k: variables[k][~to_remove].cpu().numpy() for k in SE.VARIABLE_KEYS}
    params, variables = SE.remove_points(to_remove, params, variables, opt)
    for k in KEYS:
        assert np.array_equal(params[k].detach().cpu().numpy(), exp[k]) and np.array_equal(opt.state[params[k]]["exp_avg"].cpu().numpy(), exp_m[k])
    for k in SE.VARIABLE_KEYS:
        assert np.array_equal(variables[k].cpu().numpy(), exp_v[k])
    assert params["cam_trans"].shape == (1, 3, 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        SE.compact_append([torch.zeros(4, 3)], keep=None)
    # nothing kept / everything kept
    all_gone = torch.ones(params["means3D"].shape[0], dtype=torch.bool, device="cuda")
    p2, v2 = SE.remove_points(all_gone, params, variables, opt)
    assert p2["means3D"].shape == (0, 3) and v2["timestep"].shape == (0,)


def _rank_edge_masks():
    edges = torch.zeros(257, dtype=torch.bool)
    edges[[63, 64, 255, 256]] = True     # last lane, first lane of the next wave, last thread, first thread of the next block
    return [("edges_257", edges), ("all_256", torch.ones(256, dtype=torch.bool)), ("none_256", torch.zeros(256, dtype=torch.bool))]


@pytest.mark.parametrize("name,keep", _rank_edge_masks(), ids=[n for n, _ in _rank_edge_masks()])
def test_compaction_rank_at_wave_and_block_edges(name, keep):
    """the caller-mask path of remove_points (count, scan, rank) where a rank crosses a wave or a block: rows equal tensor[mask]"""
    from hsr_utils import slam_external as SE
    P = keep.shape[0]
    g = torch.Generator().manual_seed(P)
    tensors = [torch.rand(P, 3, generator=g), torch.rand(P, generator=g), torch.arange(P, dtype=torch.float32)[:, None].repeat(1, 4)]
    got = SE.compact_append([t.cuda() for t in tensors], keep=keep.to(torch.uint8).cuda())
    for t, o in zip(tensors, got):
        assert o.shape == t[keep].shape and torch.equal(o.cpu(), t[keep])


# ---- gradient-driven densification (utils/slam_external.py:191-242; off in the reference's configs).  Pinned by the reference's own outputs at
# the end of this file (tests/golden/slam_helpers/densify_gradient.npz).  The restatement below (accumulate, clone-concat, split-concat, remove
# the split originals, prune, reset, written with plain concatenations and boolean indexing) is itself held to that fixture on the CPU
# (tests/test_slam_helpers_golden.py) and serves here for what the reference cannot do: larger maps, 26 semantic columns, a carried 'timestep'.
# Both sides draw ONE torch.normal of the same shape under the same seed. ----
def _densify_stepwise(params, moments, variables, it, dd, grad2d, seen):
    """dicts of plain tensors in, dicts out; `moments[k]` = (exp_avg, exp_avg_sq)"""
    keys = list(KEYS)
    acc, den = variables["means2D_gradient_accum"].clone(), variables["denom"].clone()
    acc[seen] += grad2d[seen, :2].norm(dim=-1)
    den[seen] += 1
    out_vars = dict(variables, means2D_gradient_accum=acc, denom=den)
    if it >= dd["start_after"] and it % dd["densify_every"] == 0:
        g = acc / den
        g[g.isnan()] = 0.0
        R = variables["scene_radius"]
        big = lambda ls: torch.exp(ls).max(dim=1).values
        clone = (g >= dd["grad_thresh"]) & (big(params["log_scales"]) <= 0.01 * R)
        P0 = params["means3D"].shape[0]
        cat = lambda d, new: {k: torch.cat((d[k], new[k])) for k in keys}
        zeros_like_rows = lambda new: {k: (torch.zeros_like(new[k]), torch.zeros_like(new[k])) for k in keys}
        catm = lambda m, z: {k: (torch.cat((m[k][0], z[k][0])), torch.cat((m[k][1], z[k][1]))) for k in keys}
        new = {k: params[k][clone] for k in keys}
        has_t = "timestep" in variables         # the reference's densify cannot carry the key (its fixtures leave it out); the repository's can
        tstep = torch.cat((variables["timestep"], variables["timestep"][clone])) if has_t else torch.zeros(P0 + int(clone.sum()), device=g.device)
        params, moments = cat(params, new), catm(moments, zeros_like_rows(new))
        P1 = params["means3D"].shape[0]
        gp = torch.zeros(P1, device=g.device)
        gp[:P0] = g
        split = (gp >= dd["grad_thresh"]) & (big(params["log_scales"]) > 0.01 * R)
        n = dd["num_to_split_into"]
        new = {k: params[k][split].repeat(n, 1) for k in keys}
        std = torch.exp(params["log_scales"])[split]
        std = (std if std.shape[1] == 3 else std.repeat(1, 3)).repeat(n, 1)
        samples = torch.normal(mean=torch.zeros_like(std), std=std)
        q = torch.nn.functional.normalize(params["unnorm_rotations"][split]).repeat(n, 1)
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        rot = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                           2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                           2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
        new["means3D"] = new["means3D"] + torch.bmm(rot, samples.unsqueeze(-1)).squeeze(-1)
        new["log_scales"] = torch.log(torch.exp(new["log_scales"]) / (0.8 * n))
        tstep = torch.cat((tstep, tstep[split].repeat(n)))
        params, moments = cat(params, new), catm(moments, zeros_like_rows(new))
        P2 = params["means3D"].shape[0]
        gone = torch.cat((split, torch.zeros(P2 - P1, dtype=torch.bool, device=split.device)))
        take = lambda keep: ({k: params[k][keep] for k in keys}, {k: (moments[k][0][keep], moments[k][1][keep]) for k in keys})
        params, moments = take(~gone)
        tstep = tstep[~gone]
        thr = dd["final_removal_opacity_threshold"] if it == dd["stop_after"] else dd["removal_opacity_threshold"]
        gone = (torch.sigmoid(params["logit_opacities"]) < thr).squeeze(-1)
        if it >= dd["remove_big_after"]:
            gone = gone | (big(params["log_scales"]) > 0.1 * R)
        params, moments = take(~gone)
        tstep = tstep[~gone]
        rows = params["means3D"].shape[0]
        zero = torch.zeros(rows, device=g.device)
        out_vars = dict(variables, means2D_gradient_accum=zero, denom=zero.clone(), max_2D_radius=zero.clone(), **({"timestep": tstep} if has_t else {}),
                        _counts=(int(clone.sum()), int(split.sum()), P2 - int(gone.sum()) - int(split.sum()) - rows + int(gone.sum())))
    if it > 0 and it % dd["reset_opacities_every"] == 0 and dd["reset_opacities"]:
        params = dict(params, logit_opacities=torch.log(torch.full_like(params["logit_opacities"], 0.01) / 0.99))
        moments = dict(moments, logit_opacities=(torch.zeros_like(params["logit_opacities"]), torch.zeros_like(params["logit_opacities"])))
    return params, moments, out_vars


@pytest.mark.parametrize("it, remove_big, reset", [(100, False, False), (300, True, False), (500, True, True), (150, False, False),
                                                    (700, False, False)])
def test_gradient_driven_densify_matches_its_stepwise_restatement(it, remove_big, reset):
    from hsr_utils import slam_external as SE
    z = np.load(GOLD, allow_pickle=False)
    params, variables, opt = _load_state(z, "prune_iter0/in")
    P = params["means3D"].shape[0]
    g = torch.Generator().manual_seed(it)
    variables["means2D_gradient_accum"] = (torch.rand(P, generator=g) * 2e-3).cuda()
    variables["denom"] = torch.randint(0, 4, (P,), generator=g).float().cuda()       # zeros -> 0/0 = NaN -> 0
    variables["seen"] = (torch.rand(P, generator=g) < 0.6).cuda()
    variables["scene_radius"] = torch.tensor(float(torch.exp(params["log_scales"].detach()).max(dim=1).values.median()) / 0.01 * 1.0).cuda()
    m2d = torch.zeros(P, 3, device="cuda", requires_grad=True)
    m2d.grad = (torch.randn(P, 3, generator=g) * 1e-3).cuda()
    variables["means2D"] = m2d
    dd = dict(start_after=100, remove_big_after=300, stop_after=500, densify_every=100, grad_thresh=6e-4, num_to_split_into=2,
              removal_opacity_threshold=0.3, final_removal_opacity_threshold=0.5, reset_opacities=reset, reset_opacities_every=250)
    plain = {k: params[k].detach().clone() for k in KEYS}
    mom = {k: (opt.state[params[k]]["exp_avg"].clone(), opt.state[params[k]]["exp_avg_sq"].clone()) for k in KEYS}
    var0 = {k: (v.clone() if torch.is_tensor(v) and k != "means2D" else v) for k, v in variables.items()}
    torch.manual_seed(1234)
    exp_p, exp_m, exp_v = _densify_stepwise(plain, mom, var0, it, dd, m2d.grad, variables["seen"])
    torch.manual_seed(1234)
    params, variables = SE.densify(params, variables, opt, it, dd)
    if it > dd["stop_after"]:
        assert params["means3D"].shape[0] == P and torch.equal(variables["denom"], var0["denom"])      # nothing happens any more
        return
    assert params["means3D"].shape[0] == exp_p["means3D"].shape[0]
    if it % 100 == 0:
        n_clone, n_split, _ = exp_v["_counts"]
        assert n_clone > 20 and n_split > 20 and params["means3D"].shape[0] < P + n_clone + n_split   # it really clones, splits and prunes
    for k in KEYS:
        a, e = params[k].detach(), exp_p[k]
        if k == "means3D":
            assert torch.allclose(a, e, rtol=0, atol=2e-6 * float(e.abs().max())), k     # R v by cross products vs by a rotation matrix
        else:
            assert torch.equal(a, e), k
        st = opt.state[params[k]]
        assert torch.equal(st["exp_avg"], exp_m[k][0]) and torch.equal(st["exp_avg_sq"], exp_m[k][1]), k
        assert [g_ for g_ in opt.param_groups if g_["name"] == k][0]["params"][0] is params[k]
    for k in ("means2D_gradient_accum", "denom", "max_2D_radius", "timestep"):
        assert torch.equal(variables[k], exp_v[k]), k
    assert params["cam_trans"].shape == (1, 3, 5)
    (params["means3D"].sum() + params["semantic"].sum()).backward()      # the densified map still trains through the re-keyed state
    opt.step()


@pytest.mark.parametrize("grad_thresh, removal, expect", [(1e9, 0.3, "prune_only"), (6e-4, 1.1, "empty_map"), (1e9, -1.0, "nothing")])
def test_gradient_driven_densify_edge_cases(grad_thresh, removal, expect):
    """nothing exceeds the gradient threshold (only the closing prune acts); every Gaussian falls below the opacity threshold (the
    map becomes empty and still trains); neither (the map is unchanged, accumulators restart)"""
    from hsr_utils import slam_external as SE
    z = np.load(GOLD, allow_pickle=False)
    params, variables, opt = _load_state(z, "prune_iter0/in")
    P = params["means3D"].shape[0]
    g = torch.Generator().manual_seed(9)
    variables["means2D_gradient_accum"] = (torch.rand(P, generator=g) * 2e-3).cuda()
    variables["denom"] = torch.randint(1, 4, (P,), generator=g).float().cuda()
    variables["seen"] = (torch.rand(P, generator=g) < 0.6).cuda()
    variables["scene_radius"] = torch.tensor(1e6).cuda()
    m2d = torch.zeros(P, 3, device="cuda", requires_grad=True)
    m2d.grad = (torch.randn(P, 3, generator=g) * 1e-3).cuda()
    variables["means2D"] = m2d
    before = {k: params[k].detach().clone() for k in KEYS}
    op = torch.sigmoid(before["logit_opacities"]).squeeze(-1)
    dd = dict(start_after=100, remove_big_after=10 ** 9, stop_after=500, densify_every=100, grad_thresh=grad_thresh, num_to_split_into=2,
              removal_opacity_threshold=removal, final_removal_opacity_threshold=removal, reset_opacities=False, reset_opacities_every=250)
    params, variables = SE.densify(params, variables, opt, 200, dd)
    n = params["means3D"].shape[0]
    if expect == "prune_only":
        keep = op >= removal
        assert n == int(keep.sum()) and 0 < n < P
        for k in KEYS:
            assert torch.equal(params[k].detach(), before[k][keep]), k
    elif expect == "empty_map":
        assert n == 0 and all(params[k].shape[0] == 0 for k in KEYS) and variables["denom"].shape == (0,)
    else:
        assert n == P
        for k in KEYS:
            assert torch.equal(params[k].detach(), before[k]), k
    assert variables["denom"].shape == (n,) and not bool(variables["means2D_gradient_accum"].any())
    assert params["cam_trans"].shape == (1, 3, 5)
    (params["means3D"].sum() + params["semantic"].sum()).backward()
    opt.step()


# ---- the gradient-driven densify against the REFERENCE's own outputs: tests/golden/slam_helpers/densify_gradient.npz holds what
# utils/slam_external.densify returns on the CPU for a map whose torch.optim.Adam state comes from two real steps, with the samples its one
# torch.normal call drew (tests/golden/make_slam_helpers_golden.py); read through tests/slam_helpers_fixture.py ----
def _fixture_cases():
    import slam_helpers_fixture as GF
    return GF.densify_cases()


class _TorchWithRecordedNormal:
    """what hsr_utils.slam_external sees as `torch` during the test: torch itself, but normal() hands out the reference's draw"""

    def __init__(self, normal):
        self.normal = normal

    def __getattr__(self, name):
        return getattr(torch, name)


@pytest.mark.parametrize("name", _fixture_cases())
def test_gradient_driven_densify_matches_the_reference_outputs(name, monkeypatch):
    """Bit-equal to the reference: the row count and order, every tensor whose rows are only moved (colours, rotations, opacities, semantics,
    the kept and cloned rows of means3D and log_scales), both Adam moments, `step`, the zeroed accumulators; which rows were cloned and
    which split, read from a row-id column that the repository's densify carries as 'timestep'.  The split rows' means3D and log_scales go
    through a rotation product and log(exp(.) / (0.8 n)) on the device: bit-equal, or at most twice as far from a float64 restatement as
    the reference's fp32 values are (the criterion of tests/test_gpu_map_init.py).  On an accumulate-only iteration the accumulator is
    sqrt(gx^2 + gy^2) added by torch on either side: three correctly rounded operations that a fused multiply-add may contract, held to 3
    ulp (3.6e-7 relative)."""
    import slam_helpers_fixture as GF
    from hsr_utils import slam_external as SE
    params, variables, opt, it, dd, draw, exp = GF.densify_case(name, device="cuda")
    P = params["means3D"].shape[0]
    densifies = it <= dd["stop_after"] and it >= dd["start_after"] and it % dd["densify_every"] == 0
    ids64 = f64 = None
    if densifies:                                        # float64 restatement on the CPU, with a row-id column
        cp, cv, copt = GF.densify_case(name)[:3]
        plain, mom = GF.plain_state(cp, copt)
        plain = {k: v.double() for k, v in plain.items()}
        var0 = {k: v for k, v in cv.items() if k != "means2D"}
        var0["timestep"] = torch.arange(P, dtype=torch.float64)
        with monkeypatch.context() as m:
            m.setattr(torch, "normal", GF.RecordedNormal(draw))
            f64, _, v64 = _densify_stepwise(plain, mom, var0, it, dd, cv["means2D"].grad, cv["seen"])
        ids64 = v64["timestep"].long().numpy()
    normal = GF.RecordedNormal(draw)
    monkeypatch.setattr(SE, "torch", _TorchWithRecordedNormal(normal))
    variables["timestep"] = torch.arange(P, device="cuda", dtype=torch.float32)
    params, variables = SE.densify(params, variables, opt, it, dd)
    assert normal.calls == int(draw is not None and draw.shape[0] > 0)
    rows = exp["param/means3D"].shape[0]
    assert params["means3D"].shape[0] == rows
    ids = variables["timestep"].cpu().numpy().astype(np.int64)
    if densifies:
        assert np.array_equal(ids, ids64), "another set of rows was kept, cloned or split"
        z_in = GF.load("densify_gradient.npz")["%s/param/log_scales" % str(GF.load("densify_gradient.npz")[name + "/state"])]
        split_row = (exp["param/log_scales"].view(np.uint32) != z_in[ids].view(np.uint32)).any(axis=1)
    else:
        assert np.array_equal(ids, np.arange(P))
        split_row = np.zeros(rows, bool)
    for i, k in enumerate(GF.DKEYS):
        got, want = params[k].detach().cpu().numpy(), exp["param/" + k]
        assert isinstance(params[k], torch.nn.Parameter) and params[k].requires_grad and got.shape == want.shape
        if k in ("means3D", "log_scales"):
            assert np.array_equal(got[~split_row], want[~split_row]), k
            if split_row.any():
                ref = f64[k].numpy()
                exact = np.array_equal(got, want)
                d_kernel, d_ref = float(np.abs(got - ref).max()), float(np.abs(want - ref).max())
                print("densify %-22s %-10s %4d split rows  bit-equal to the reference: %-5s  |device - f64| %.3e   |reference - f64| %.3e"
                      % (name, k, int(split_row.sum()), exact, d_kernel, d_ref))
                assert exact or d_kernel <= 2.0 * d_ref, (name, k, d_kernel, d_ref)
        else:
            assert np.array_equal(got, want), k
        st = opt.state[params[k]]
        assert np.array_equal(st["exp_avg"].cpu().numpy(), exp["exp_avg/" + k]) and np.array_equal(st["exp_avg_sq"].cpu().numpy(), exp["exp_avg_sq/" + k]), k
        assert float(st["step"]) == exp["step"][i]
        assert [g_ for g_ in opt.param_groups if g_["name"] == k][0]["params"][0] is params[k]
    for k in ("cam_unnorm_rots", "cam_trans"):
        assert np.array_equal(params[k].detach().cpu().numpy(), exp["param/" + k])
    assert len(opt.state) == 8
    for k in GF.DVARS + ("seen", "scene_radius"):
        got, want = variables[k].cpu().numpy(), exp["var/" + k]
        if k == "means2D_gradient_accum" and not densifies:
            np.testing.assert_allclose(got, want, rtol=3.6e-7, atol=0, err_msg=k)
        else:
            assert np.array_equal(got, want), k
    print("densify %-22s rows %d -> %d, %d of them split products: order, moved rows, moments, step and accumulators equal the reference's"
          % (name, P, rows, int(split_row.sum())))
    (params["means3D"].sum() + params["semantic"].sum()).backward()      # the densified map still trains through the re-keyed state
    opt.step()
