"""GPU suite for hsr_utils.export.export_frame / hsr_frame_export (include/ext/hsr_frame_export.h) and evaluate.evaluate_sequence: every
picture is compared BIT FOR BIT with the numpy restatement of the header, tests/export_ref.py (which tests/test_frame_export_cpu.py shows
to agree with a literal restatement of the reference's lines), on the input lists of that module laid into images: all 255 exact
rounding ties of the colour rule, the values whose depth index sits on the edge of truncation, out-of-range labels, tied logits.  Sizes:
1x1, 1x3, 3x5, 37x53 (H * W % 4 = 1: planes off 16 bytes, a one-pixel tail) and 5x205 (1025 pixels: one past whole 4-pixel groups and
256-lane blocks), each also with every input taken from a view one element into its storage, which makes the call take the
one-pixel-per-lane variant."""
import os

import numpy as np
import pytest
import torch

import export_ref as X
import test_frame_export_cpu as XC

pytestmark = pytest.mark.gpu

SIZE_IDS = ["%dx%d" % s for s in X.SIZES]
LOGIT_SIZES, LOGIT_K = (3, 5, 8, 6), 26      # 22 planes in levels, 4 trailing planes that are never read


def _dev(a, offset):
    """the array on the device; with offset, as a view one element into a larger allocation: same values, a pointer off 16 bytes"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.cuda()
    big = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    view = big[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


def _tables():
    from hsr_utils.export import jet_colormap, label_colormap
    g = np.random.default_rng(4)
    return dict(jet=jet_colormap("cpu").numpy(), label=label_colormap(40, "cpu").numpy(),
                tuples=g.integers(1, 256, size=(int(np.prod(LOGIT_SIZES)), 3)).astype(np.uint8))      # no black row: black means refused


def _logit_planes(shape):
    """float32 [26,H,W]: per level, values apart by at least 0.25 or exactly equal — exact ties between two planes, all planes of a level
    equal — and NaN in the 4 planes past the levels"""
    g = np.random.default_rng(shape[0] * 1000 + shape[1])
    x = (g.integers(-8, 9, size=(LOGIT_K,) + shape) * 0.25).astype(np.float32)      # a grid of quarters: many exact ties of the maximum
    flat = x.reshape(LOGIT_K, -1)
    flat[:, ::7] = 1.5                    # every plane equal: label 0 on every level
    flat[3:8, 1::7] = -2.0
    flat[[4, 6], 1::7] = 0.75             # level 1 (planes 3..7): planes 4 and 6 tie for the maximum, the lower one wins
    x[sum(LOGIT_SIZES):] = np.nan
    return x


def _level_planes(sizes, shape, seed):
    g = np.random.default_rng(seed)
    lev = np.stack([g.integers(0, s, size=shape) for s in sizes]).astype(np.int64)
    flat = lev.reshape(len(sizes), -1)
    bad = (-1, None, 1 << 40, -(1 << 40), 1 << 32, (1 << 32) + 1)      # None: the level's own size; 2^32 (+1): 0 (1) as a 32-bit word
    for k, v in enumerate(bad):
        at = np.arange(2 + 3 * k, flat.shape[1], 23)
        l = k % len(sizes)
        flat[l, at] = sizes[l] if v is None else v
    return lev


@pytest.fixture(scope="module")
def tables():
    host = _tables()
    return host, {k: torch.from_numpy(v).cuda() for k, v in host.items()}


def _same(got, want):
    assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == want.shape
    g = got.cpu().numpy()
    assert np.array_equal(g, want), "first difference at flat byte %d of %d" % (int(np.flatnonzero(g.reshape(-1) != want.reshape(-1))[0]), want.size)


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("shape", X.SIZES, ids=SIZE_IDS)
def test_every_kind_matches_the_restatement_bit_for_bit(shape, offset, tables):
    from hsr_utils.export import export_frame
    host, dev = tables
    level_sizes = list(LOGIT_SIZES) + [99]
    cv, dv = X.colour_values(), X.depth_values()
    im, gt_im = X.lay(cv, (3,) + shape), X.lay(cv[::-1].copy(), (3,) + shape, shift=5)
    depth, gt_depth = X.lay(dv, shape), X.lay(dv, shape, shift=131)
    lab = X.lay(np.array([0, 39, 40, -1, 7, 2 ** 31 - 1, -2 ** 31, 12, 38, 1], dtype=np.int32), shape)
    gt_lab = X.lay(np.array([3, 1 << 40, 39, 40, -1, 0, (1 << 32) + 5, 17], dtype=np.int64), shape)      # int64 labels: one level of 40
    sem, gt_levels = _logit_planes(shape), _level_planes(LOGIT_SIZES, shape, 21)
    out = export_frame(im=_dev(im, offset), gt_im=_dev(gt_im, offset), depth=_dev(depth[None], offset), gt_depth=_dev(gt_depth, offset),
                       im_semantic=_dev(sem, offset), gt_levels=_dev(gt_levels, offset), labels=_dev(lab, offset),
                       gt_labels=_dev(gt_lab[None], offset), level_sizes=level_sizes, tuple_table=dev["tuples"], label_table=dev["label"])
    assert list(out) == ["im", "gt_im", "depth", "gt_depth", "im_semantic", "gt_levels", "labels", "gt_labels"]
    _same(out["im"], X.color(im))
    _same(out["gt_im"], X.color(gt_im))
    _same(out["depth"], X.depth(depth, host["jet"]))
    _same(out["gt_depth"], X.depth(gt_depth, host["jet"]))
    _same(out["im_semantic"], X.logits(sem, LOGIT_SIZES, host["tuples"]))
    _same(out["gt_levels"], X.levels(gt_levels, LOGIT_SIZES, host["tuples"]))
    _same(out["labels"], X.labels(lab, host["label"]))
    _same(out["gt_labels"], X.labels(gt_lab, host["label"]))
    if shape == (37, 53):
        assert out["im_semantic"].cpu().numpy().reshape(-1, 3).any(axis=1).all()                   # every logit pixel found a tuple
        assert not X.levels(gt_levels, LOGIT_SIZES, host["tuples"]).reshape(-1, 3).any(axis=1).all()      # and some gt tuples are refused
    # eight jobs in one launch give the bytes of eight launches of one job
    if offset is False:
        single = dict(im=im, gt_im=gt_im, depth=depth, gt_depth=gt_depth, im_semantic=sem, gt_levels=gt_levels, labels=lab, gt_labels=gt_lab)
        for key, a in single.items():
            one = export_frame(level_sizes=level_sizes, tuple_table=dev["tuples"], label_table=dev["label"], **{key: _dev(a, False)})
            assert list(one) == [key] and torch.equal(one[key], out[key]), key


@pytest.mark.parametrize("lo,hi", [(0.0, 6.0), (0.5, 3.25), (-2.0, 1e-3)])
def test_depth_ranges_and_a_callers_table(lo, hi, tables):
    from hsr_utils.export import export_frame
    dv = X.depth_values()
    depth = X.lay(dv, (7, 61), shift=2)
    depth[3] = depth[3] * np.float32(0.5) + np.float32(lo)
    own = np.random.default_rng(8).integers(0, 256, size=(256, 3)).astype(np.uint8)
    out = export_frame(depth=_dev(depth, False), depth_range=(lo, hi), depth_table=torch.from_numpy(own).cuda())
    _same(out["depth"], X.depth(depth, own, lo, hi))


@pytest.mark.parametrize("sizes", [(5,), (3, 4, 2, 6), (1, 2) * 8], ids=["L1", "L4", "L16"])
def test_levels_of_1_4_and_16(sizes, tables):
    from hsr_utils.export import export_frame
    n = int(np.prod(sizes))
    table = np.random.default_rng(len(sizes)).integers(1, 256, size=(n, 3)).astype(np.uint8)
    lev = _level_planes(sizes, (9, 29), 5 + len(sizes))
    want = X.levels(lev, sizes, table)
    black = ~want.reshape(-1, 3).any(axis=1)
    assert black.any() and not black.all()
    out = export_frame(gt_levels=_dev(lev, False), level_sizes=list(sizes) + [3], tuple_table=torch.from_numpy(table).cuda())
    _same(out["gt_levels"], want)
    x = (np.random.default_rng(6).integers(-8, 9, size=(sum(sizes),) + (9, 29)) * 0.25).astype(np.float32)
    out = export_frame(im_semantic=_dev(x, False), level_sizes=list(sizes) + [3], tuple_table=torch.from_numpy(table).cuda())
    _same(out["im_semantic"], X.logits(x, sizes, table))


@pytest.mark.parametrize("shape", [(37, 53), (5, 205)], ids=["37x53", "5x205"])
def test_logits_equal_the_levels_picture_of_semantic_labels(shape, tables):
    """the level labels are hsr_eval_labels_tree's, bit for bit, on logits with near ties that only the fp32 softmax decides"""
    from hsr_utils import evaluate
    from hsr_utils.export import export_frame
    host, dev = tables
    g = np.random.default_rng(shape[1])
    x = g.normal(size=(LOGIT_K,) + shape).astype(np.float32) * 3
    flat = x.reshape(LOGIT_K, -1)
    flat[1, ::3] = flat[0, ::3] + np.float32(3e-8)                   # within the 1e-6 pre-test: expf and the division decide
    flat[9, 1::3] = np.maximum(flat[8, 1::3], flat[10, 1::3]) + np.float32(5e-7)
    flat[16:22, 2::5] = flat[16, 2::5]                               # the last level all equal
    flat[8:16, 3::11] = np.float32(80.0) * np.arange(8, dtype=np.float32)[:, None]      # differences that underflow expf
    x[sum(LOGIT_SIZES):] = np.nan
    level_sizes = list(LOGIT_SIZES) + [99]
    xd = torch.from_numpy(x).cuda()
    tree_table = torch.zeros(int(np.prod(LOGIT_SIZES)), dtype=torch.int32, device="cuda")
    _leaf, levels = evaluate.semantic_labels(xd, "tree", level_sizes=level_sizes, tree_table=tree_table)
    a = export_frame(im_semantic=xd, level_sizes=level_sizes, tuple_table=dev["tuples"])["im_semantic"]
    b = export_frame(gt_levels=levels.long(), level_sizes=level_sizes, tuple_table=dev["tuples"])["gt_levels"]
    assert torch.equal(a, b)
    assert a.cpu().numpy().reshape(-1, 3).any(axis=1).all()
    big = torch.empty(x.size + 1, dtype=torch.float32, device="cuda")
    big[1:].copy_(xd.reshape(-1))
    c = export_frame(im_semantic=big[1:].view(xd.shape), level_sizes=level_sizes, tuple_table=dev["tuples"])["im_semantic"]
    assert torch.equal(c, b)                                        # and the one-pixel-per-lane variant


def test_an_output_off_4_bytes_takes_the_other_variant_with_the_same_bytes(tables):
    """the C entry point itself: one COLOR job into out + 1"""
    from diff_gaussian_rasterization import _abi
    shape = (5, 205)
    im = X.lay(X.colour_values(), (3,) + shape)
    src = torch.from_numpy(im).cuda()
    out = torch.full((shape[0] * shape[1] * 3 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    job = (_abi.hsr_export_job * 1)(_abi.hsr_export_job(kind=0, src=src.data_ptr(), out=out.data_ptr() + 1))
    _abi.call(_abi.lib.hsr_frame_export, "hsr_frame_export", src.device, shape[0], shape[1], 1, job)
    got = out.cpu().numpy()
    assert got[0] == 0xA5 and (got[1 + 3 * 1025:] == 0xA5).all()
    assert np.array_equal(got[1:1 + 3 * 1025].reshape(5, 205, 3), X.color(im))


@pytest.mark.parametrize("kind", range(5))
def test_refusals_leave_the_output_untouched(kind, tables):
    """every refusal of the header (the list of the CPU suite, here with device pointers and a valid job of each kind as the base):
    the error code, and the canary-filled output unchanged; then the base itself writes every byte"""
    from diff_gaussian_rasterization import _abi
    H = W = 8
    out = torch.full((H * W * 3,), 0xA5, dtype=torch.uint8, device="cuda")
    src = torch.zeros(16 * H * W, dtype=torch.int64, device="cuda")      # zeros are valid input of every kind
    table = torch.ones((256, 3), dtype=torch.uint8, device="cuda")
    base = [dict(kind=0), dict(kind=1, n=256), dict(kind=2, n=256), dict(kind=3, L=3, sizes=(4, 8, 8), n=256),
            dict(kind=4, L=3, sizes=(4, 8, 8), n=256, K=20)][kind]
    base.update(src=src.data_ptr(), table=table.data_ptr(), out=out.data_ptr())
    refused = 0
    with torch.cuda.device(out.device):
        for kw, message in XC.REFUSALS:
            if "job" in kw and kw["job"]["kind"] in range(5) and kw["job"]["kind"] != kind:
                continue      # a refusal of another kind's fields
            rc = XC.refused_call(_abi.lib, base, **kw)
            assert rc == -1 and message in _abi.lib.hsr_last_error(), (kw, rc, _abi.lib.hsr_last_error())
            refused += 1
        torch.cuda.synchronize()
        assert bool((out == 0xA5).all()) and refused >= 12
        assert XC.refused_call(_abi.lib, base) == 0
        torch.cuda.synchronize()
    assert not bool((out == 0xA5).any())


def test_wrapper_checks_launch_nothing_and_one_call_is_one_launch(monkeypatch, tables):
    from hsr_utils import export
    _host, dev = tables
    calls = []
    real = export._lib.hsr_frame_export
    monkeypatch.setattr(export._lib, "hsr_frame_export", lambda *a: calls.append(a) or real(*a))
    im = torch.zeros(3, 4, 6, device="cuda")
    with pytest.raises(RuntimeError, match=r"gt_im must be \[3,4,6\]"):
        export.export_frame(im=im, gt_im=torch.zeros(3, 4, 7, device="cuda"))
    with pytest.raises(RuntimeError, match="depth must be"):
        export.export_frame(im=im, depth=torch.zeros(1, 4, 7, device="cuda"))
    with pytest.raises(RuntimeError, match="must be torch.float32"):
        export.export_frame(im=im.double())
    with pytest.raises(RuntimeError, match="gt_levels must be torch.int64"):
        export.export_frame(gt_levels=torch.zeros(4, 4, 6, dtype=torch.int32, device="cuda"), level_sizes=[3, 5, 8, 6, 9], tuple_table=dev["tuples"])
    with pytest.raises(RuntimeError, match="tuple_table must be uint8"):
        export.export_frame(gt_levels=torch.zeros(4, 4, 6, dtype=torch.int64, device="cuda"), level_sizes=[3, 5, 8, 7, 9], tuple_table=dev["tuples"])
    with pytest.raises(RuntimeError, match="K >= 22"):
        export.export_frame(im_semantic=torch.zeros(21, 4, 6, device="cuda"), level_sizes=[3, 5, 8, 6, 9], tuple_table=dev["tuples"])
    with pytest.raises(RuntimeError, match="depth_table must be uint8"):
        export.export_frame(depth=im[:1], depth_table=dev["label"])
    assert calls == []
    out = export.export_frame(im=im, gt_im=im, depth=im[0], gt_depth=im[:1])
    assert len(calls) == 1 and calls[0][2] == 4 and sorted(out) == ["depth", "gt_depth", "gt_im", "im"]


# ---- evaluate_sequence: a 3-frame synthetic semantic session at 176x168 ---------------------------------------------------------------
W, H, LEVELS, FRAMES, K = 176, 168, [2, 2], 3, 4
SCALE = 6553.5
TREE = {0: (0, 0), "1": (0, 1), 2: (1, 0), 3: (1, 1)}
LEVEL_SIZES = LEVELS + [4]      # the levels, then the leaf count
COLOURS = {(0, 0): (255, 0, 0), (0, 1): (0, 255, 0), (1, -1): (0, 0, 255)}


def _hidden_map(kmat):
    """the hidden surface of tests/test_gpu_slam_session_multires.py for this size: colours and labels that vary over the image"""
    from hsr_utils import make_scene
    P = 135000
    sc = make_scene(P, W, H, K, kmat, seed=7, kind="slam")
    fx, fy, cx, cy = kmat[0][0], kmat[1][1], kmat[0][2], kmat[1][2]
    g = torch.Generator().manual_seed(8)
    u = torch.rand(P, generator=g) * (W + 96) - 48
    v = torch.rand(P, generator=g) * (H + 96) - 48
    z = 2.5 + 0.35 * torch.sin(u / 18.0) + 0.25 * torch.cos(v / 14.0)
    means = torch.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], dim=1).float()
    colour = 0.5 + 0.25 * torch.stack([torch.sin(u / 10.0), torch.cos(v / 8.0), torch.sin((u + v) / 12.0)], dim=1) + 0.25 * (sc["colors_precomp"] - 0.5)
    sem = sc["semantics_precomp"].clone()
    sem[:, 0] += (u > W / 2).float()
    sem[:, 2] += (v > H / 2).float()
    scale = (1.3 * z / (0.5 * (fx + fy))).float()
    return {"means3D": means, "rgb_colors": colour.float().clamp(0, 1), "unnorm_rotations": sc["rotations"],
            "logit_opacities": torch.full((P, 1), 3.0), "log_scales": scale.log()[:, None], "semantic": sem}


@pytest.fixture(scope="module")
def session():
    """(the stepped session, its frames as ingest() built them, the camera, the tables)"""
    import random
    import test_gpu_slam_session_multires as M
    from diff_gaussian_rasterization import GaussianRasterizer_semantic
    from hsr_utils import SlamSession, evaluate, export, setup_camera, slam, slam_helpers as SH, tree_label_table
    from hsr_utils.camera import replica_intrinsics
    kmat = replica_intrinsics(W, H)
    cam = setup_camera(W, H, kmat, np.eye(4), device="cuda")
    hidden = {k: v.cuda().contiguous() for k, v in _hidden_map(kmat).items()}
    rots, trans = M._gt_path()
    hidden["cam_unnorm_rots"], hidden["cam_trans"] = rots[..., :FRAMES].contiguous().cuda(), trans[..., :FRAMES].contiguous().cuda()
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    cfg = M._config(5, sizes=None)
    cfg["data"]["num_frames"] = FRAMES
    cfg["data"]["png_depth_scale"] = SCALE
    cfg["mapping"]["num_iters"] = 5
    s = SlamSession(cfg, torch.tensor(kmat, dtype=torch.float32, device="cuda"), torch.eye(4, device="cuda"), cam)
    table = tree_label_table(TREE, 2, device="cuda")
    frames = []
    with torch.no_grad():
        raw = []
        for t in range(FRAMES):
            rv = SH.transformed_params2rendervar_semantic(hidden, SH.transform_to_frame(hidden, t, False, False))
            im, _radius, sem, depth, _median, _opac = GaussianRasterizer_semantic(raster_settings=cam)(**rv)
            color_u8 = (im.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
            depth_u16 = (depth[0] * SCALE).round().clamp(0, 32767).to(torch.int16)
            ids = (2 * sem[:2].argmax(dim=0) + sem[2:4].argmax(dim=0)).to(torch.uint8)
            raw.append((color_u8, depth_u16, ids, slam.frame_w2c(hidden, t)))
    for t, (color_u8, depth_u16, ids, gt_w2c) in enumerate(raw):
        frame = s.ingest(t, color_u8, depth_u16, gt_w2c=gt_w2c, labels=ids, tree_table=table)
        s.step(frame)
        frames.append(frame)
    tabs = dict(level_sizes=LEVEL_SIZES, tree_table=evaluate.tree_lookup_table(TREE, LEVEL_SIZES), num_classes=4,
                tuple_table=export.tuple_colour_table(COLOURS, LEVEL_SIZES, True))
    return s, frames, cam, tabs


def test_evaluate_sequence_scores_files_and_pictures(session, tmp_path):
    from PIL import Image
    from hsr_utils import evaluate, export
    s, frames, cam, tabs = session
    eval_dir = str(tmp_path / "eval")
    sil = 0.5
    result = evaluate.evaluate_sequence(s.params, (f for f in frames), cam, eval_dir, sil_thres=sil, mapping_iters=5, add_new_gaussians=True,
                                        mode="tree", save_frames=True, **tabs)
    assert result["frame_ids"] == [0, 1, 2]
    files = dict(psnr="psnr.txt", depth_rmse="rmse.txt", depth_l1="l1.txt", ms_ssim="ssim.txt", miou="miou.txt", mbiou="mbiou.txt")
    assert sorted(n for n in os.listdir(eval_dir) if n.endswith(".txt")) == sorted(list(files.values()) + ["summary.txt"])
    written = {k: np.loadtxt(os.path.join(eval_dir, name)) for k, name in files.items()}
    kw = {k: tabs[k] for k in ("level_sizes", "tree_table", "num_classes")}
    names = dict(im="rendered_rgb/gs_%04d.png", depth="rendered_depth/gs_%04d.png", gt_im="rgb/gt_%04d.png", gt_depth="depth/gt_%04d.png",
                 im_semantic="rendered_semantic/sem_%04d_multilevel.png", gt_levels="rendered_semantic/gt_%04d.png")
    for row, frame in enumerate(frames):
        im, depth, _opac, sem = s.render(frame["id"])
        want = evaluate.evaluate_frame(im, frame["im"], depth, frame["depth"], sem, frame["semantic_label_gt"][-1], "tree", ms_ssim=True, **kw)
        for k in files:
            assert written[k].shape == (3,) and written[k][row] == float(want[k]) == result[k][row], (k, row, written[k][row], float(want[k]))
            assert np.isfinite(written[k][row])
        pictures = export.export_frame(im=im, gt_im=frame["im"], depth=depth, gt_depth=frame["depth"], im_semantic=sem,
                                       gt_levels=frame["semantic_label_gt"][:-1], level_sizes=LEVEL_SIZES, tuple_table=tabs["tuple_table"])
        for key, pattern in names.items():
            with Image.open(os.path.join(eval_dir, pattern % frame["id"])) as png:
                assert png.mode == "RGB" and np.array_equal(np.asarray(png), pictures[key].cpu().numpy()), (key, row)
        colours = {tuple(c) for c in pictures["gt_levels"].cpu().numpy().reshape(-1, 3).tolist()}
        assert colours == {(255, 0, 0), (0, 255, 0), (0, 0, 255)}      # the hidden map shows every class; (1, -1) covers two of them
    for k in files:
        assert result["avg_" + k] == float(result[k].mean())
    assert np.isfinite(result["ate_rmse"]) and result["ate_rmse"] == evaluate.trajectory_ate([f["gt_w2c"] for f in frames], s.estimated_w2c())
    assert sum(len(os.listdir(os.path.join(eval_dir, d))) for d in ("rendered_rgb", "rendered_depth", "rgb", "depth")) == 12
    assert len(os.listdir(os.path.join(eval_dir, "rendered_semantic"))) == 6


def test_evaluate_sequence_eval_every_the_silhouette_branch_and_no_mode(session, tmp_path):
    from hsr_utils import evaluate
    s, frames, cam, tabs = session
    sil = 0.5
    kw = {k: tabs[k] for k in ("level_sizes", "tree_table", "num_classes")}
    # eval_every = 2 scores frames 0 and 1 only: frame 0 always, then (id + 1) % 2 == 0; the silhouette enters with mapping_iters == 0
    # and no new Gaussians
    result = evaluate.evaluate_sequence(s.params, frames, cam, str(tmp_path / "every2"), eval_every=2, sil_thres=sil, mapping_iters=0,
                                        add_new_gaussians=False, mode="tree", ms_ssim=False, **kw)
    assert result["frame_ids"] == [0, 1] and "ms_ssim" not in result
    assert sorted(os.listdir(str(tmp_path / "every2"))) == ["l1.txt", "mbiou.txt", "miou.txt", "psnr.txt", "rmse.txt", "summary.txt"]
    assert np.loadtxt(str(tmp_path / "every2" / "psnr.txt")).shape == (2,)
    for row, t in enumerate((0, 1)):
        im, depth, opac, sem = s.render(t)
        want = evaluate.evaluate_frame(im, frames[t]["im"], depth, frames[t]["depth"], sem, frames[t]["semantic_label_gt"][-1], "tree",
                                       final_opacity=opac, sil_thres=sil, **kw)
        assert all(result[k][row] == float(want[k]) for k in want)
    assert np.isfinite(result["ate_rmse"])      # every frame's pose counts, scored or not
    # no mode: the loop of eval_newrender — the plain rasterizer, no semantic scores, nothing written without a directory
    plain = evaluate.evaluate_sequence(s.params, frames, cam, sil_thres=sil, mapping_iters=5, add_new_gaussians=True, mode=None)
    assert plain["frame_ids"] == [0, 1, 2] and "miou" not in plain and plain["psnr"].shape == (3,) and np.isfinite(plain["avg_ms_ssim"])
    with pytest.raises(RuntimeError, match="save_frames needs eval_dir"):
        evaluate.evaluate_sequence(s.params, frames, cam, sil_thres=sil, mapping_iters=5, add_new_gaussians=True, mode=None, save_frames=True)
