"""GPU parity for the keyframe selection (include/hsr_keyframes.h, hsr_utils/keyframes.py): the committed outputs of the reference's own
keyframe_selection_overlap (tests/golden/keyframes/*.npz) under its seeds, the rounding key against torch.round on the device, the rank
selection against torch.where, and a full-size frame with 400 keyframes against tests/keyframe_ref.py in float64 under the borderline
rule stated there."""
import glob
import os

import numpy as np
import pytest
import torch

import keyframe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "keyframes", "*.npz")))
NAMES = [os.path.basename(p)[:-4] for p in FIXTURES]
pytestmark = pytest.mark.gpu


def _kf():
    from hsr_utils import keyframes as KF
    return KF


def _load(path):
    d = np.load(path)
    dev = lambda k: torch.tensor(d[k]).cuda()
    return d, dev("depth"), dev("w2c"), dev("intrinsics"), dev("est_w2c")


def _as_list(poses):
    return [{'est_w2c': m, 'id': 5 * i} for i, m in enumerate(poses)]


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_fixtures_reproduce_the_reference(path):
    KF = _kf()
    d, depth, w2c, K, poses = _load(path)
    k, pixels = int(d["k"]), int(d["pixels"])
    torch.manual_seed(int(d["torch_seed"]))
    counts, n_pts, pts, pix, keep = KF.overlap_counts(depth, w2c, K, _as_list(poses), pixels, details=True)
    print(os.path.basename(path), "counts", counts.cpu().numpy().tolist(), "reference", d["counts"].tolist(), "b", d["borderline"].tolist())
    assert np.array_equal(pix.cpu().numpy(), d["sampled_pixels"])
    assert np.array_equal(keep.cpu().numpy(), d["keep"])
    assert int(n_pts) == d["pts"].shape[0]
    np.testing.assert_allclose(pts[:int(n_pts)].cpu().numpy(), d["pts"], rtol=0, atol=2e-5)   # a few fp32 ulps of coordinates below 16
    assert (np.abs(counts.cpu().numpy().astype(np.int64) - d["counts"]) <= d["borderline"]).all()
    torch.manual_seed(int(d["torch_seed"]))
    np.random.seed(int(d["numpy_seed"]))
    got = KF.keyframe_selection_overlap(depth, w2c, K, _as_list(poses), k, pixels)
    assert [int(i) for i in got] == d["selected"].tolist()
    assert all(isinstance(i, np.integer) for i in got)


def test_round_keys_match_torch_round_on_the_device():
    KF = _kf()
    g = torch.Generator().manual_seed(3)
    halves = (torch.arange(-2000, 2000, dtype=torch.float64) + 0.5) * 1e-4
    mags = torch.logspace(-5, 3, 4001, dtype=torch.float64)
    vals = torch.cat([torch.tensor([0.0, -0.0, 5e-5, -5e-5, 4.99999e-5, 1.5e-4, 2.5e-4, 1e-5, 1e3], dtype=torch.float64), halves,
                      halves * 100, mags, -mags, (torch.rand(20000, generator=g, dtype=torch.float64) - 0.5) * 20,
                      torch.randn(20000, generator=g, dtype=torch.float64) * 300]).float().cuda()
    got = KF.round_keys(vals)
    exp = torch.round(vals, decimals=4).abs()
    assert torch.equal(got, exp), (vals[got != exp][:8], got[got != exp][:8], exp[got != exp][:8])
    assert not torch.signbit(got).any()


def _depth_cases():
    g = np.random.default_rng(9)
    for H, W in ((41, 41), (96, 128), (340, 600), (680, 1200)):
        d = (g.random((H, W)) * 4 + 0.5).astype(np.float32)
        d[g.random((H, W)) < 0.3] = 0.0
        d[g.random((H, W)) < 0.02] = -1.0                     # negative depth is invalid too
        d[0] = 0.0
        d[H // 3:H // 3 + 4] = 0.0                            # rows with no valid pixel
        d[H - 1] = 0.0
        yield "holes_%dx%d" % (H, W), d
        one = np.zeros((H, W), np.float32)
        one[H - 2, W - 3] = 2.0
        yield "single_%dx%d" % (H, W), one
        yield "all_%dx%d" % (H, W), np.full((H, W), 1.5, np.float32)


@pytest.mark.parametrize("name,depth", list(_depth_cases()), ids=[n for n, _ in _depth_cases()])
def test_rank_selection_matches_torch_where(name, depth):
    KF = _kf()
    d = torch.tensor(depth).cuda()[None]
    H, W = depth.shape
    valid = R.valid_pixels(d)
    n_valid = valid.shape[0]
    prefix = KF.valid_row_prefix(d)
    exp_prefix = torch.cat([torch.zeros(1, dtype=torch.int64, device=d.device), (d[0] > 0).sum(dim=1).cumsum(0)])
    assert torch.equal(prefix.long(), exp_prefix) and int(prefix[H]) == n_valid
    g = torch.Generator().manual_seed(H + W)
    ranks = torch.cat([torch.tensor([0, n_valid - 1]), torch.randint(n_valid, (4094,), generator=g)])
    if n_valid <= 4096:
        ranks = torch.arange(n_valid)
    K = torch.tensor([[W / 2.0, 0, W / 2.0], [0, W / 2.0, H / 2.0], [0, 0, 1]])
    pts, pix, keep, count = KF.sample_points(d, torch.eye(4).cuda(), K, ranks)
    exp = valid[ranks.cuda()]
    assert torch.equal(pix.long(), exp)
    # identity pose: the points are the camera-space ones, operation for operation (:17-22).  The intrinsics go to the device first, as
    # the reference holds them: dividing a device tensor by a HOST scalar, torch multiplies by the reciprocal, which is another rounding
    z = d[0, exp[:, 0], exp[:, 1]]
    K = K.cuda()
    cam = torch.stack((((exp[:, 1].float() - K[0, 2]) / K[0, 0]) * z, ((exp[:, 0].float() - K[1, 2]) / K[1, 1]) * z, z), dim=-1)
    exp_keep = R.keep_by_keys(cam)
    assert torch.equal(keep.bool(), exp_keep) and int(count) == int(exp_keep.sum())
    assert torch.equal(pts[:int(count)], cam[exp_keep])


@pytest.mark.parametrize("H,W", [(1025, 3), (2049, 1)])
def test_row_scan_with_more_rows_than_scan_threads(H, W):
    """hsr_kf_valid_rows where the single-workgroup scan holds two and three counts per thread: all H + 1 words against numpy.cumsum"""
    KF = _kf()
    g = np.random.default_rng(H)
    depth = (g.random((H, W)) * 4 + 0.5).astype(np.float32)
    bad = g.random((H, W)) < 0.3
    depth[bad] = np.where(g.random((H, W)) < 0.5, 0.0, -1.0).astype(np.float32)[bad]      # about 30 % non-positive
    prefix = KF.valid_row_prefix(torch.tensor(depth).cuda()[None]).cpu().numpy()
    exp = np.concatenate([[0], np.cumsum((depth > 0).sum(axis=1))])
    assert prefix.shape == (H + 1,) and np.array_equal(prefix.astype(np.int64), exp)


def _rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    x, y, z = axis
    Kx = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def _pose(Rm, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm, t
    return T


def _trajectory(n_kf, H, W, seed=0):
    """a room seen from a camera that turns once around while it drifts: most keyframes overlap the current view partly, a third
    look away"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (2.5 + 0.8 * np.sin(5.0 * xx / W + 1.0) + 0.6 * np.cos(3.0 * yy / H)).astype(np.float32)
    depth[g.random((H, W)) < 0.1] = 0.0
    depth[100:110] = 0.0
    K = np.array([[W / 2.0, 0, W / 2.0 - 0.5], [0, W / 2.0, H / 2.0 - 0.5], [0, 0, 1]], np.float32)
    w2c = _pose(_rot([0.2, 1.0, 0.1], 0.4), [0.1, -0.2, 0.3])
    poses = []
    for i in range(n_kf):
        a = 2 * np.pi * i / n_kf
        rel = _pose(_rot([0.1 * np.sin(3 * a), 1.0, 0.05], a) @ _rot([1, 0, 0], 0.15 * np.sin(5 * a)), [0.8 * np.sin(a), 0.1 * np.cos(2 * a), 0.5 * (1 - np.cos(a))])
        poses.append(rel @ w2c)
    f32 = lambda m: torch.tensor(np.asarray(m, np.float32))
    return f32(depth[None]), f32(w2c), f32(K), torch.stack([f32(m) for m in poses])


def test_full_size_400_keyframes_against_float64():
    KF = _kf()
    H, W, n_kf, pixels = 680, 1200, 400, 1600
    depth, w2c, K, poses = _trajectory(n_kf, H, W)
    dd, dw, dK, dp = depth.cuda(), w2c.cuda(), K.cuda(), poses.cuda()
    torch.manual_seed(5)
    counts, n_pts, pts, pix, keep = KF.overlap_counts(dd, dw, dK, _as_list(dp), pixels, details=True)
    torch.manual_seed(5)
    again = KF.overlap_counts(dd, dw, dK, _as_list(dp), pixels, details=True)
    n = int(n_pts)
    for a, b in zip((counts, n_pts, pts[:n], pix, keep), (again[0], again[1], again[2][:n], again[3], again[4])):
        assert torch.equal(a, b)                                             # bit-identical runs
    torch.manual_seed(5)
    ranks = torch.randint(int((depth[0] > 0).sum()), (pixels,))
    sampled = R.valid_pixels(depth)[ranks]
    assert torch.equal(pix.cpu().long(), sampled)
    keep64 = R.keep_by_pixels(sampled, R.back_project(depth, K, w2c, sampled))
    assert torch.equal(keep.cpu().bool(), keep64) and n == int(keep64.sum())
    pts64 = R.back_project(depth, K, w2c, sampled, torch.float64)[keep64]
    inside64, border, _u, _v, _m = R.borderline(pts64, poses, K, W, H)
    c64, b = inside64.sum(dim=1).numpy(), border.sum(dim=1).numpy()
    got = counts.cpu().numpy().astype(np.int64)
    print("full size: %d points, counts min %d max %d, %d keyframes with count 0, borderline pairs %d, keyframes off float64 %d" % (
        n, got.min(), got.max(), int((got == 0).sum()), int(b.sum()), int((got != c64).sum())))
    assert b.sum() <= 5e-4 * border.numel()
    assert (np.abs(got - c64) <= b).all(), np.nonzero(np.abs(got - c64) > b)
    assert (got == 0).sum() >= 20 and (got > n // 2).sum() >= 20               # the trajectory exercises both ends
    # the points themselves: fp32 (back-projection, the fp32 inverse) against float64, within the rule's 64 * 2^-24 of the largest coordinate
    assert float((pts[:n].cpu().double() - pts64).abs().max()) <= R.TAU * float(pts64.abs().max())


def test_list_and_table_inputs_agree():
    KF = _kf()
    d, depth, w2c, K, poses = _load(FIXTURES[-2])
    k, pixels = 6, int(d["pixels"])
    table = KF.KeyframePoses(device=depth.device, capacity=4)
    for m in poses:
        table.append(m)
    assert len(table) == poses.shape[0] and torch.equal(table.table(), poses)
    out = []
    for kfl, n in ((_as_list(poses)[:-1], None), (table, len(table) - 1), (_as_list(poses), len(table) - 1)):
        torch.manual_seed(1)
        np.random.seed(2)
        out.append([int(i) for i in KF.keyframe_selection_overlap(depth, w2c, K, kfl, k, pixels, n_keyframes=n)])
    assert out[0] == out[1] == out[2] and len(out[0]) == k and max(out[0]) < len(table) - 1
    torch.manual_seed(1)
    c_list = KF.overlap_counts(depth, w2c, K, _as_list(poses), pixels)[0]
    torch.manual_seed(1)
    c_table = KF.overlap_counts(depth, w2c, K, table, pixels)[0]
    assert torch.equal(c_list, c_table)


def test_edge_cases():
    KF = _kf()
    d, depth, w2c, K, poses = _load(FIXTURES[0])
    pixels = int(d["pixels"])
    # an empty keyframe list returns [] after drawing the ranks
    torch.manual_seed(4)
    np.random.seed(4)
    assert KF.keyframe_selection_overlap(depth, w2c, K, [], 5, pixels) == []
    state = torch.get_rng_state()
    torch.manual_seed(4)
    torch.randint(int((depth[0] > 0).sum()), (pixels,))
    assert torch.equal(torch.get_rng_state(), state)
    # no valid depth pixel: torch.randint's own error, as in the reference (:58)
    with pytest.raises(RuntimeError) as ours:
        KF.keyframe_selection_overlap(torch.zeros_like(depth), w2c, K, _as_list(poses), 5, pixels)
    with pytest.raises(RuntimeError) as theirs:
        torch.randint(0, (pixels,))
    assert str(ours.value) == str(theirs.value)
    # k larger than the candidates: every keyframe with a non-zero count, none with zero
    torch.manual_seed(int(d["torch_seed"]))
    got = KF.keyframe_selection_overlap(depth, w2c, K, _as_list(poses), 1000, pixels)
    assert sorted(int(i) for i in got) == np.nonzero(d["counts"] > 0)[0].tolist()
    # more sampled pixels than one workgroup's table holds
    with pytest.raises(RuntimeError, match="4096"):
        KF.keyframe_selection_overlap(depth, w2c, K, _as_list(poses), 5, pixels=5000)


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_rng_streams_advance_as_the_restatement_advances_them(path):
    KF = _kf()
    d, depth, w2c, K, poses = _load(path)
    k, pixels = int(d["k"]), int(d["pixels"])
    states = []
    for fn, args in ((KF.keyframe_selection_overlap, (depth, w2c, K, _as_list(poses))),
                     (R.keyframe_selection_overlap, (depth.cpu(), w2c.cpu(), K.cpu(), _as_list(poses.cpu())))):
        torch.manual_seed(int(d["torch_seed"]))
        np.random.seed(int(d["numpy_seed"]))
        torch.cuda.manual_seed(77)
        dev_state = torch.cuda.get_rng_state()
        sel = fn(*args, k, pixels)
        states.append(([int(i) for i in sel], torch.get_rng_state(), np.random.get_state()[1].copy(), int(np.random.get_state()[2])))
        assert torch.equal(torch.cuda.get_rng_state(), dev_state)             # the device generator is not touched
    assert states[0][0] == states[1][0]
    assert torch.equal(states[0][1], states[1][1]) and np.array_equal(states[0][2], states[1][2]) and states[0][3] == states[1][3]


def test_selected_window_sees_the_current_surface():
    """a short synthetic sequence through the loop's two lines (scripts/hierslam.py:1966-1974): every selected keyframe really sees part of
    the current frame's surface (float64), none that sees nothing is selected, and the window ends with the last keyframe and the frame"""
    KF = _kf()
    H, W, n_frames = 240, 320, 30
    depth, _w2c, K, poses = _trajectory(n_frames, H, W, seed=2)
    table, keyframe_list = KF.KeyframePoses(device="cuda"), []
    torch.manual_seed(0)
    np.random.seed(0)
    for t in range(n_frames):
        cur = poses[t].cuda()
        if t > 0:
            state = torch.get_rng_state()
            selected = KF.keyframe_selection_overlap(depth.cuda(), cur, K.cuda(), table, 8, 600, n_keyframes=len(table) - 1)
            after = torch.get_rng_state()
            torch.set_rng_state(state)
            sampled = R.valid_pixels(depth)[torch.randint(int((depth[0] > 0).sum()), (600,))]
            torch.set_rng_state(after)
            keep = R.keep_by_pixels(sampled, R.back_project(depth, K, poses[t], sampled))
            pts64 = R.back_project(depth, K, poses[t], sampled, torch.float64)[keep]
            cand = torch.stack([kf['est_w2c'].cpu() for kf in keyframe_list[:-1]]) if len(keyframe_list) > 1 else torch.zeros(0, 4, 4)
            if cand.shape[0]:
                inside64, border, *_ = R.borderline(pts64, cand, K, W, H)
                sure = (inside64 & ~border).sum(dim=1).numpy()
                maybe = (inside64 | border).sum(dim=1).numpy()
                assert all(maybe[int(i)] > 0 for i in selected)
                if len(selected) < 8:
                    assert set(np.nonzero(sure > 0)[0].tolist()) <= set(int(i) for i in selected)
            else:
                assert selected == []
            ids, window = KF.mapping_window(selected, keyframe_list, t)
            assert window[-1] == -1 and ids[-1] == t and window[-2] == len(keyframe_list) - 1 and len(window) <= 10
        keyframe_list.append({'id': t, 'est_w2c': cur})
        table.append(cur)
