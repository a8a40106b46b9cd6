"""The optimizer step on the device (include/hsr_optim.h, hsr_utils/optim.py) against what the reference runs: torch.optim.Adam with its
defaults, i.e. the foreach path on a HIP device.  One step from identical state, a 200-step trajectory, the fallback bookkeeping,
state_dict interchange, the map-surgery loop with both optimizers side by side, and the tracking loop's best-pose candidate."""
import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HEADLINE_P, HEADLINE_K, HEADLINE_T = 500_000, 26, 2000
SPECIAL = torch.tensor([0.0, -0.0, 1e-40, -3e-42, 1e-20, -1e-20, 1e20, -1e20, math.inf, -math.inf, math.nan])


def _ordered(t):
    """fp32 bits as integers ordered like the floats (ulp distance = difference)"""
    i = t.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def _diff(a, b):
    """(elements that differ, largest ulp distance among finite pairs); non-finite values must be classified identically"""
    a, b = a.detach().reshape(-1), b.detach().reshape(-1)
    assert torch.equal(torch.isnan(a), torch.isnan(b)), "NaN positions differ"
    assert torch.equal(torch.isposinf(a), torch.isposinf(b)) and torch.equal(torch.isneginf(a), torch.isneginf(b)), "inf positions differ"
    fin = torch.isfinite(a)
    ulp = (_ordered(a[fin]) - _ordered(b[fin])).abs()          # -0.0 and +0.0 are 0 ulp apart here, but their bits differ
    differ = a[fin].view(torch.int32) != b[fin].view(torch.int32)
    return int(differ.sum()), int(ulp.max()) if ulp.numel() else 0


def _assert_bit_identical(what, got, exp):
    n, worst = _diff(got, exp)
    assert n == 0, "%s: %d of %d elements differ from torch, worst %d ulp" % (what, n, got.numel(), worst)


def _shapes_small():
    out = [(0,), (1,), (3,), (7,), (1023,)]
    out += [(50_000, c) for c in (1, 3, 4, 26, 102)]
    return out


def _headline_shapes(K=HEADLINE_K, P=HEADLINE_P, T=HEADLINE_T):
    return [(P, 3), (P, 3), (P, 4), (P, 1), (P, 1), (P, K), (1, 4, T), (1, 3, T)]


def _make_pair(shapes, groups_kw, seed, odd_grads, dev="cuda"):
    """the same params / grads / state for an hsr Adam and a torch Adam.  odd_grads: every grad a view at an odd float offset of one
    flat buffer (16-byte misaligned), else own allocations.  Special values are planted in every grad of 16+ elements."""
    from hsr_utils.optim import Adam
    g = torch.Generator(device="cpu").manual_seed(seed)
    ps = [torch.randn(s, generator=g) for s in shapes]
    total = sum(int(np.prod(s)) for s in shapes)
    flat = (torch.randn(total + 2 * len(shapes) + 1, generator=g) * 1e-3).to(dev)
    grads, off = [], 1
    for s in shapes:
        n = int(np.prod(s))
        gr = flat[off:off + n].view(s) if odd_grads else flat[off:off + n].clone().view(s)
        off += n + (2 if odd_grads else 0)
        if n >= 16:
            gr.view(-1)[3:3 + SPECIAL.numel()] = SPECIAL.to(dev)
        grads.append(gr)
    state = [(float(3 + i % 4), torch.randn(s, generator=g) * 1e-3, torch.rand(s, generator=g) * 1e-6) for i, s in enumerate(shapes)]
    opts, sets = [], []
    for cls in (Adam, torch.optim.Adam):
        mine = [p.to(dev).requires_grad_(True) for p in ps]
        k = 0
        groups = []
        for kw, n in groups_kw:
            groups.append(dict(params=mine[k:k + n], **kw))
            k += n
        assert k == len(mine)
        opt = cls(groups)
        for p, gr, (st, m, v) in zip(mine, grads, state):
            p.grad = gr
            opt.state[p] = {"step": torch.tensor(st), "exp_avg": m.to(dev), "exp_avg_sq": v.to(dev)}
        opts.append(opt)
        sets.append(mine)
    return opts, sets


def _compare(opts, sets, what):
    for i, (a, b) in enumerate(zip(*sets)):
        _assert_bit_identical("%s param %d %s" % (what, i, tuple(a.shape)), a, b)
        sa, sb = opts[0].state[a], opts[1].state[b]
        assert torch.equal(sa["step"], sb["step"]) and not sa["step"].is_cuda
        _assert_bit_identical("%s exp_avg %d" % (what, i), sa["exp_avg"], sb["exp_avg"])
        _assert_bit_identical("%s exp_avg_sq %d" % (what, i), sa["exp_avg_sq"], sb["exp_avg_sq"])


@pytest.mark.parametrize("lr,eps", [(1e-3, 1e-8), (0.05, 1e-15), (0.0, 1e-15), (0.0, 1e-8)])
@pytest.mark.parametrize("odd", [False, True])
def test_one_step_matches_torch_adam(lr, eps, odd):
    shapes = _shapes_small()
    (mine, ref), sets = _make_pair(shapes, [({"lr": lr, "eps": eps}, len(shapes))], seed=1, odd_grads=odd)
    mine.step(); ref.step()
    assert mine.last_fused_tensors == len(shapes) and mine.last_fused_numel == sum(int(np.prod(s)) for s in shapes)
    _compare((mine, ref), sets, "lr=%g eps=%g odd=%s" % (lr, eps, odd))


@pytest.mark.parametrize("K", [HEADLINE_K, 102])
def test_one_step_headline_map(K):
    """the mapping optimizer of the reference (:411-417: lr 0 default, eps 1e-15) on the whole map plus the camera tensors"""
    shapes = _headline_shapes(K)
    lrs = [1e-4, 2.5e-3, 1e-3, 0.05, 1e-3, 2.5e-3, 0.0, 0.0]
    (mine, ref), sets = _make_pair(shapes, [({"lr": lr, "eps": 1e-15}, 1) for lr in lrs], seed=2, odd_grads=False)
    mine.step(); ref.step()
    assert mine.last_fused_tensors == len(shapes)
    _compare((mine, ref), sets, "headline K=%d" % K)


def test_table_longer_than_one_launch():
    shapes = [(97 + 5 * i,) for i in range(45)]            # 45 tensors: two launches of the library
    (mine, ref), sets = _make_pair(shapes, [({"lr": 1e-2}, 45)], seed=3, odd_grads=True)
    mine.step(); ref.step()
    assert mine.last_fused_tensors == 45
    _compare((mine, ref), sets, "45 tensors")


def _traj_model(seed, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).to(dev).requires_grad_(True) for s in ((4000, 3), (4000, 26), (4000, 1), (1, 4, 10))]


def _traj_grads(params, it, dead_rows):
    g = torch.Generator().manual_seed(1000 + it)
    out = []
    for k, p in enumerate(params):
        gr = (torch.randn(p.shape, generator=g) * 10.0 ** (-(it % 4))).to(p.device)
        if p.dim() == 2:
            gr[dead_rows] = 0.0                          # Gaussians that are never visible: zero gradient, moments still decay
        out.append(None if (k == 3 and it % 3 == 1) else gr)   # the camera tensor skips every third step: its own step count
    return out


# bounds for two runs of the same trajectory: identical arithmetic gives identical bits; these fp32 bounds are what the check allows
TRAJ_REL = 1e-6


def _run_trajectory(switches=None):
    """run `a` with hsr Adam (or with the classes of `switches`, {iteration: class}, handing the state over by state_dict) and `b`
    with torch.optim.Adam on the same gradients"""
    from hsr_utils.optim import Adam
    switches = switches or {}
    a, b = _traj_model(7), _traj_model(7)
    dead = torch.arange(0, 4000, 7)
    groups = lambda ps: [{"params": ps[:3], "lr": 1e-2, "eps": 1e-15}, {"params": ps[3:], "lr": 4e-4}]
    oa, ob = switches.get(0, Adam)(groups(a)), torch.optim.Adam(groups(b))
    for it in range(200):
        if it == 120:                                    # a learning-rate change mid-run
            for o in (oa, ob):
                o.param_groups[0]["lr"] = 2e-3
        if it in switches and it > 0:
            sd = oa.state_dict()
            oa = switches[it](groups(a)); oa.load_state_dict(sd)
            assert type(oa) is switches[it]
        gs = _traj_grads(a, it, dead)
        for p, q, gr in zip(a, b, gs):
            p.grad = None if gr is None else gr.clone()
            q.grad = None if gr is None else gr.clone()
        if it % 25 == 0:                                 # the one-step check from shared state, on the way
            c = [p.detach().clone().requires_grad_(True) for p in a]
            oc = torch.optim.Adam(groups(c)); oc.load_state_dict(copy.deepcopy(oa.state_dict()))   # (loading aliases the tensors)
            for p, q in zip(a, c):
                q.grad = None if p.grad is None else p.grad.clone()
            oc.step()
        oa.step(); ob.step()
        if it % 25 == 0:
            _compare((oa, oc), (a, c), "trajectory step %d" % it)
        for p, q in zip(a, b):
            tol = TRAJ_REL * (1.0 + q.detach().abs())
            assert bool(((p - q).abs() <= tol).all()), it
    assert oa.state[a[3]]["step"].item() != oa.state[a[0]]["step"].item()
    for p, q in zip(a, b):
        _assert_bit_identical("trajectory end", p, q)
    init = _traj_model(7)
    for k in range(3):                                   # rows that never saw a gradient: zero moments, the step adds -0
        assert torch.equal(a[k][dead], init[k][dead]) and not bool(oa.state[a[k]]["exp_avg"][dead].any())


def test_trajectory_200_steps():
    _run_trajectory()


def test_state_dict_interchange_mid_run():
    from hsr_utils.optim import Adam
    _run_trajectory({0: torch.optim.Adam, 90: Adam, 150: torch.optim.Adam})


def test_bookkeeping_and_fallbacks():
    from hsr_utils.optim import Adam
    g = torch.Generator().manual_seed(11)

    def model():
        g.manual_seed(11)
        return {"a": torch.randn(300, 3, generator=g).cuda(), "b": torch.randn(257, generator=g).cuda(),
                "none": torch.randn(50, generator=g).cuda(), "ams": torch.randn(64, generator=g).cuda(),
                "wd": torch.randn(64, generator=g).cuda(), "max": torch.randn(64, generator=g).cuda(),
                "f64": torch.randn(64, generator=g, dtype=torch.float64).cuda(), "strided": torch.randn(32, 64, generator=g).cuda()}

    def groups(m):
        return [{"params": [m["a"], m["b"], m["none"], m["f64"], m["strided"]], "lr": 1e-2},
                {"params": [m["ams"]], "amsgrad": True}, {"params": [m["wd"]], "weight_decay": 0.1},
                {"params": [m["max"]], "maximize": True}]

    ma, mb = model(), model()
    for m in (ma, mb):
        for v in m.values():
            v.requires_grad_(True)
    oa, ob = Adam(groups(ma)), torch.optim.Adam(groups(mb))
    none_before = ma["none"].detach().clone()
    for it in range(5):
        g.manual_seed(50 + it)
        for k in ma:
            if k == "none":
                continue
            if k == "strided":                                    # a grad with other strides than its param
                gr = torch.randn(64, 32, generator=g).cuda().t()
            else:
                gr = torch.randn(ma[k].shape, generator=g, dtype=ma[k].dtype).cuda()
            ma[k].grad, mb[k].grad = gr, gr.clone()
        oa.step(); ob.step()
        assert oa.last_fused_tensors == 2 and oa.last_fused_numel == 900 + 257
        for k in ma:
            assert torch.equal(ma[k], mb[k]), (it, k)
    assert torch.equal(ma["none"], none_before) and ma["none"] not in oa.state
    for k in ma:
        if k != "none":
            for n, t in ob.state[mb[k]].items():
                assert torch.equal(oa.state[ma[k]][n], t), (k, n)


def test_step_on_a_side_stream_and_without_host_sync():
    from hsr_utils.optim import Adam
    shapes = [(100_000, 3), (7,)]
    (mine, ref), sets = _make_pair(shapes, [({"lr": 1e-3}, 2)], seed=4, odd_grads=True)
    for p in sets[0]:
        mine.state.pop(p)                                         # lazy state creation inside the checked region too
    for p in sets[1]:
        ref.state.pop(p)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(s):
            mine.step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.current_stream().wait_stream(s)
    ref.step()
    torch.cuda.synchronize()
    _compare((mine, ref), sets, "side stream")


# ------------------------------------------------------------------------------------------------------------- map surgery
def test_mapping_with_map_surgery_both_optimizers():
    """the surgery scenario of test_gpu_slam_loop.py with torch.optim.Adam and hsr Adam side by side: one render + backward per
    iteration (on the torch run's map) feeds both, so the two maps see the same gradients and must stay equal through prune and
    densify (the backward's fp32 atomics would otherwise make two renders differ in the last bits)."""
    import test_gpu_slam_loop as SL
    from hsr_utils import losses as L, slam_external as SE, slam_helpers as SH
    from hsr_utils.optim import Adam
    from diff_gaussian_rasterization import GaussianRasterizer_semantic
    cam, params, (W, H, K) = SL._scene(P=12000)
    params["cam_unnorm_rots"] = torch.tensor([1.0, 0, 0, 0]).view(1, 4, 1).cuda()
    params["cam_trans"] = torch.zeros(1, 3, 1).cuda()
    with torch.no_grad():
        im_gt, _, sem_gt, depth_gt, _, _ = SL._render(params, cam, 0, False, False)
    sizes = [4, 8]
    lab = torch.stack([sem_gt[:4].argmax(dim=0), sem_gt[4:12].argmax(dim=0)])
    g = torch.Generator().manual_seed(5)
    for k in ("means3D", "rgb_colors", "semantic", "logit_opacities", "log_scales"):
        params[k] = (params[k] + 0.05 * torch.randn(params[k].shape, generator=g).cuda() * params[k].abs().mean())
    lrs = {"means3D": 1e-4, "rgb_colors": 2.5e-3, "unnorm_rotations": 1e-3, "semantic": 2.5e-3, "logit_opacities": 0.05, "log_scales": 1e-3,
           "cam_unnorm_rots": 0.0, "cam_trans": 0.0}
    P0 = params["means3D"].shape[0]
    runs = []
    for cls in (torch.optim.Adam, Adam):
        ps = {k: torch.nn.Parameter(v.detach().clone().requires_grad_(True)) for k, v in params.items()}
        opt = cls([{"params": [ps[k]], "name": k, "lr": lrs[k]} for k in ps], lr=0.0, eps=1e-15)    # hierslam.py:417
        var = {"means2D_gradient_accum": torch.zeros(P0).cuda(), "denom": torch.zeros(P0).cuda(), "max_2D_radius": torch.zeros(P0).cuda(),
               "timestep": torch.zeros(P0).cuda(), "scene_radius": torch.tensor(float(depth_gt.max()) / 3.0).cuda()}
        runs.append([ps, opt, var])
    dd = dict(start_after=5, remove_big_after=10 ** 9, stop_after=10 ** 9, densify_every=10, grad_thresh=2e-5, num_to_split_into=2,
              removal_opacity_threshold=0.03, final_removal_opacity_threshold=0.03, reset_opacities=False, reset_opacities_every=10 ** 9)
    pd = dict(start_after=0, remove_big_after=10 ** 9, stop_after=10 ** 9, prune_every=7, removal_opacity_threshold=0.03,
              final_removal_opacity_threshold=0.03, reset_opacities=False, reset_opacities_every=10 ** 9)
    sizes_seen = set()
    for it in range(45):
        ps = runs[0][0]
        rv = SH.transformed_params2rendervar_semantic(ps, SH.transform_to_frame(ps, 0, True, False))
        rv["means2D"].retain_grad()
        im, radius, sem, depth, med, opac = GaussianRasterizer_semantic(raster_settings=cam)(**rv)
        mask = (depth_gt > 0).detach()
        loss = 0.5 * L.mapping_image_loss(im, im_gt) + L.masked_l1(depth, depth_gt, mask, "mean") + 0.01 * L.tree_cross_entropy(sem, lab, sizes)
        for r in runs:
            r[1].zero_grad(set_to_none=True)
        loss.backward()
        for k, p in runs[1][0].items():
            q = runs[0][0][k]
            p.grad = None if q.grad is None else q.grad.clone()
        for r in runs:
            r[1].step()
            r[2]["means2D"], r[2]["seen"] = rv["means2D"], radius > 0
            with torch.no_grad():
                r[0], r[2] = SE.prune_gaussians(r[0], r[2], r[1], it, pd)
            if r[0]["means3D"].shape[0] == r[2]["seen"].shape[0]:
                torch.manual_seed(100 + it)                     # the split's torch.normal draw: the same for both runs
                r[0], r[2] = SE.densify(r[0], r[2], r[1], it, dd)
        assert runs[1][1].last_fused_tensors == 6                # the six map tensors; the pose gets no gradient in mapping
        n0, n1 = runs[0][0]["means3D"].shape[0], runs[1][0]["means3D"].shape[0]
        assert n0 == n1, (it, n0, n1)
        sizes_seen.add(n0)
        for k in runs[0][0]:
            a, b = runs[0][0][k], runs[1][0][k]
            assert bool(((a - b).abs() <= TRAJ_REL * (1.0 + b.detach().abs())).all()), (it, k)
    assert len(sizes_seen) >= 3, sizes_seen
    for ps, opt, _ in runs:
        for k, v in ps.items():                                 # the optimizer owns exactly the live parameters
            gr = [gr for gr in opt.param_groups if gr["name"] == k][0]
            assert gr["params"][0] is v and len(gr["params"]) == 1
        assert set(opt.state) == {v for k, v in ps.items() if k not in ("cam_unnorm_rots", "cam_trans")}   # (the pose had no gradient)


# ------------------------------------------------------------------------------------------------------------- tracking candidate
def _host_candidate(losses, cols):
    """scripts/hierslam.py:1814-1816, :1855-1860 on host floats"""
    best, cand = float(np.float32(1e20)), None
    for l, c in zip(losses, cols):
        if l < best:
            best, cand = l, c
    return best, cand


def test_tracking_candidate_follows_the_reference_rule():
    from hsr_utils.optim import TrackingCandidate
    T, t = 5, 3
    g = torch.Generator().manual_seed(9)
    params = {"cam_unnorm_rots": torch.randn(1, 4, T, generator=g).cuda(), "cam_trans": torch.randn(1, 3, T, generator=g).cuda()}
    init = (params["cam_unnorm_rots"][0, :, t].cpu().clone(), params["cam_trans"][0, :, t].cpu().clone())
    cand = TrackingCandidate(params, t)
    seq = [5.0, 4.0, 4.0, 6.0, math.nan, 3.5, 3.5, math.inf, 2.0, math.nan, 2.5]
    cols = []
    dev_losses = [torch.tensor(l, device="cuda") for l in seq]   # (a host-to-device copy synchronises: made before the check)
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i, l in enumerate(dev_losses):
            params["cam_unnorm_rots"][0, :, t] += 1.0          # a new post-step pose every iteration
            params["cam_trans"][0, :, t] -= 0.5
            params["cam_trans"][0, :, 0] += 7.0                # other columns are not the candidate's
            cols.append((params["cam_unnorm_rots"][0, :, t].clone(), params["cam_trans"][0, :, t].clone()))
            cand.update(l)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    best, which = _host_candidate(seq, cols)
    assert float(cand.best_loss) == best == 2.0
    exp_r, exp_t = which[0].cpu(), which[1].cpu()
    assert not torch.equal(exp_r, init[0])
    assert torch.equal(cand.cam_unnorm_rot.cpu().view(4), exp_r) and torch.equal(cand.cam_tran.cpu().view(3), exp_t)
    other = params["cam_trans"][0, :, 0].clone()
    cand.restore(params)
    assert torch.equal(params["cam_unnorm_rots"][0, :, t].cpu(), exp_r) and torch.equal(params["cam_trans"][0, :, t].cpu(), exp_t)
    assert torch.equal(params["cam_trans"][0, :, 0], other)
    # a NaN first loss keeps the constructor's clone and the 1e20 best loss
    c2 = TrackingCandidate(params, 1)
    before = params["cam_trans"][0, :, 1].clone()
    params["cam_trans"][0, :, 1] += 1.0
    c2.update(torch.tensor(math.nan, device="cuda"))
    assert torch.equal(c2.cam_tran.view(3), before) and float(c2.best_loss) == float(np.float32(1e20))


def test_tracking_recovers_the_camera_pose_with_hsr_adam_and_candidate():
    """test_gpu_slam_loop.test_tracking_recovers_the_camera_pose with hsr Adam and TrackingCandidate, under its assertions"""
    import test_gpu_slam_loop as SL
    from hsr_utils import losses as L
    from hsr_utils.optim import Adam, TrackingCandidate
    cam, params, (W, H, K) = SL._scene()
    gt_q = torch.tensor([0.9990, 0.020, -0.030, 0.025]); gt_q = gt_q / gt_q.norm()
    gt_t = torch.tensor([0.030, -0.020, 0.040])
    rots = torch.zeros(1, 4, 2); rots[0, 0, :] = 1.0; rots[0, :, 1] = gt_q
    trans = torch.zeros(1, 3, 2); trans[0, :, 1] = gt_t
    params["cam_unnorm_rots"], params["cam_trans"] = rots.cuda(), trans.cuda()
    with torch.no_grad():
        im_gt, _, _, depth_gt, _, _ = SL._render(params, cam, 1, False, False)
    params["cam_unnorm_rots"] = rots.clone().cuda(); params["cam_unnorm_rots"][0, :, 1] = torch.tensor([1.0, 0, 0, 0])
    params["cam_trans"] = torch.zeros(1, 3, 2).cuda()
    params["cam_unnorm_rots"].requires_grad_(True); params["cam_trans"].requires_grad_(True)
    opt = Adam([{"params": [params["cam_unnorm_rots"]], "lr": 4e-4}, {"params": [params["cam_trans"]], "lr": 2e-3}])
    cand = TrackingCandidate(params, 1)

    def pose_err():
        q = torch.nn.functional.normalize(params["cam_unnorm_rots"][0, :, 1].detach().cpu(), dim=0)
        return float(1 - abs(float((q * gt_q).sum()))), float((params["cam_trans"][0, :, 1].detach().cpu() - gt_t).norm())
    r0, t0 = pose_err()
    losses = []
    for it in range(200):
        im, radius, sem, depth, med, opac = SL._render(params, cam, 1, False, True)
        mask = ((depth_gt > 0) & (opac > 0.5)).detach()
        loss = L.masked_l1(depth, depth_gt, mask, "sum") + 0.5 * L.masked_l1(im, im_gt, mask, "sum")
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        assert opt.last_fused_tensors == 2
        cand.update(loss)
        losses.append(loss.detach())
    cand.restore(params)
    first, last = float(losses[0]), float(losses[-1])
    r1, t1 = pose_err()
    assert last < 0.2 * first, (first, last)
    assert t1 < 0.2 * t0 and r1 < 0.2 * r0, ((r0, t0), (r1, t1))
    assert float(cand.best_loss) == min(float(x) for x in losses)
    assert torch.equal(params["cam_trans"][0, :, 0].detach().cpu(), torch.zeros(3))
