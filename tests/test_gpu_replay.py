"""GPU suite for the replay of a finished run (include/ext/hsr_replay.h): hsr_replay_plan against the list of counts, hsr_replay_select
bit for bit against hsr_view_prep run on `tensor[timestep <= step]` of every input, hsr_replay_cloud bit for bit against the float32
restatement of rgbd2pcd (tests/replay_ref.py), and replay_view / replay_run end to end on a small synthetic run."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import replay_ref as R
from test_gpu_slam_session import sequence  # noqa: F401  (the fixture: six rendered frames of a hidden map)
from test_gpu_view import _view_prep, _w2c
from test_view_cpu import _rot

pytestmark = pytest.mark.gpu

POISON = -777.25
POISON_INT = -77777
ROT_PARAMS, ROT_TRANSFORMED = 0, 1
TILTED = _w2c(_rot([0.9, 0.2, -0.1], 23.0), (0.3, -0.2, 0.5))


def _device():
    return torch.device("cuda", torch.cuda.current_device())


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
def _plan(ts, T):
    """hsr_replay_plan through the C ABI: a guarded output, and scratch that holds garbage at the call"""
    from diff_gaussian_rasterization import _abi
    dev = _device()
    P = int(ts.size)
    ts_dev = torch.tensor(ts, device=dev)
    out = torch.full((T + 8,), POISON_INT, dtype=torch.int64, device=dev)
    nbytes = int(_abi.lib.hsr_replay_plan_scratch_bytes(P, T))
    scratch = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)
    _abi.call(_abi.lib.hsr_replay_plan, "hsr_replay_plan", dev, P, T, ts_dev.data_ptr() if P else None, out.data_ptr(), scratch.data_ptr(), nbytes)
    assert (out[T:] == POISON_INT).all(), "written past out_upto[T]"
    return out[:T].cpu().numpy()


def _timestep_vectors(P, T, seed):
    g = np.random.default_rng(seed)
    runs = np.sort(g.integers(0, T, P)).astype(np.float32)
    special = np.array([-3, -0.0, 2.5, np.nan, np.inf, -np.inf, T - 1, T, 1e30, 0.5, T - 1.5, T - 0.5], np.float32)
    return {"zeros": np.zeros(P, np.float32), "runs": runs, "permuted": g.permutation(runs),
            "special": np.resize(special, P) if P else np.zeros(0, np.float32)}


@pytest.mark.parametrize("T", [1, 2, 7, 1000])
@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 257, 70001])
def test_plan_counts_equal_the_restatement(P, T):
    for name, ts in _timestep_vectors(P, T, 1000 * P + T).items():
        got, want = _plan(ts, T), R.plan_counts(ts, T)
        assert got.dtype == np.int64 and np.array_equal(got, want), (name, got[:8], want[:8])
        assert (np.diff(got) >= 0).all() and (P == 0 or got[-1] <= P)


def test_plan_with_the_most_steps():
    P, T = 5000, 1 << 20
    g = np.random.default_rng(5)
    ts = g.integers(0, T, P).astype(np.float32)
    ts[:12] = np.array([-3, -0.0, 2.5, np.nan, np.inf, -np.inf, T - 1, T, 1e30, 0.5, T - 1.5, T - 0.5], np.float32)
    got = _plan(ts, T)
    with np.errstate(invalid="ignore"):      # the restatement without a million passes: a sorted search gives the same counts
        finite = np.sort(ts[ts <= np.float32(T - 1)])
    want = np.searchsorted(finite, np.arange(T, dtype=np.float32), side="right").astype(np.int64)
    for t in (0, 1, 2, 3, 77, T - 2, T - 1):      # the restatement's own expression at a few steps
        assert want[t] == int(R.select_mask(ts, t).sum())
    assert np.array_equal(got, want) and got[-1] == P - 5      # NaN, +inf, T - 0.5, T and 1e30 never show


def test_replay_plan_object():
    from hsr_utils import replay
    ts = _timestep_vectors(1000, 7, 3)["permuted"]
    plan = replay.ReplayPlan(torch.tensor(ts, device="cuda"), 7)
    assert len(plan) == 7 and plan.counts.dtype == np.int64 and np.array_equal(plan.counts, R.plan_counts(ts, 7))
    assert plan.timestep.is_cuda and np.array_equal(plan.timestep.cpu().numpy(), ts)
    empty = replay.ReplayPlan(torch.zeros(0, device="cuda"), 3)
    assert empty.counts.tolist() == [0, 0, 0]


# ---- the selection ------------------------------------------------------------------------------------------------------------------------
OUTPUTS = (("means3D", 3), ("unnorm_rotations", 4), ("rotations", 4), ("opacities", 1), ("scales", 3), ("colors", 3))
INPUTS = ("means3D", "unnorm_rotations", "logit_opacities", "log_scales", "rgb_colors", "semantic")


def _map(P, S, K, seed):
    g = np.random.default_rng(seed)
    p = {"means3D": (g.standard_normal((P, 3)) * 3).astype(np.float32), "unnorm_rotations": g.standard_normal((P, 4)).astype(np.float32),
         "logit_opacities": (g.standard_normal((P, 1)) * 2).astype(np.float32), "log_scales": (g.standard_normal((P, S)) - 3).astype(np.float32),
         "rgb_colors": g.random((P, 3)).astype(np.float32), "semantic": g.standard_normal((P, K)).astype(np.float32)}
    # what a copy that is not a bit copy would change: -0.0 and NaNs with a payload
    odd = np.array([0x80000000, 0x7FC01234, 0xFFC00001], np.uint32).view(np.float32)
    for k, row in enumerate(range(0, P, max(1, P // 7))):
        p["means3D"][row, k % 3] = odd[k % 3]
        p["rgb_colors"][row, (k + 1) % 3] = odd[(k + 1) % 3]
        if K:
            p["semantic"][row, k % K] = odd[(k + 2) % 3]
    p["means3D"][P - 1, 0] = odd[0]
    return p


def _selections(P, seed):
    """(name, timestep, step): none, all, a prefix, every third row, the last row alone, a random half with NaN timesteps among the rest"""
    g = np.random.default_rng(seed)
    base = g.integers(0, 5, P).astype(np.float32)
    prefix = np.where(np.arange(P) < P // 3 + 1, 0, 1).astype(np.float32)
    third = np.where(np.arange(P) % 3 == 0, 0, 2).astype(np.float32)
    last = np.full(P, 5, np.float32)
    last[-1] = 0
    half = np.where(g.random(P) < 0.5, 0.5, 3).astype(np.float32)
    half[::11] = np.nan
    return [("none", base, -1), ("all", base, 10), ("prefix", prefix, 0), ("every third", third, 1), ("last row", last, 0), ("random half", half, 1)]


def _select(dev_in, ts_dev, step, S, K, transform_rots, rot_source, w2c_dev, capacity, rows, nulls=()):
    """hsr_replay_select through the C ABI into poisoned buffers of `rows` rows; returns ({name: [rows,c] tensor}, index, count)"""
    from diff_gaussian_rasterization import _abi
    dev = _device()
    P = int(dev_in["means3D"].shape[0])
    bufs = {k: torch.full((rows, c), POISON, device=dev) for k, c in OUTPUTS}
    bufs["semantic"] = torch.full((rows, max(K, 1)), POISON, device=dev)
    index = torch.full((rows,), POISON_INT, dtype=torch.int32, device=dev)
    count = torch.full((1,), POISON_INT, dtype=torch.int32, device=dev)
    nbytes = int(_abi.lib.hsr_replay_select_scratch_bytes(P))
    scratch = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)
    ptr = lambda name, t: None if name in nulls or t.numel() == 0 else t.data_ptr()
    _abi.call(_abi.lib.hsr_replay_select, "hsr_replay_select", dev, P, S, K, int(transform_rots), rot_source, int(step), int(capacity),
              ts_dev.data_ptr(), *[ptr("in_" + k, dev_in[k]) for k in INPUTS], None if w2c_dev is None else w2c_dev.data_ptr(),
              *[ptr(k, bufs[k]) for k in ("means3D", "unnorm_rotations", "rotations", "opacities", "scales", "colors")],
              ptr("semantic", bufs["semantic"]) if K else None, ptr("index", index), count.data_ptr(), scratch.data_ptr(), nbytes)
    return bufs, index, int(count.item())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_selection(P, K, S, seed):
    inp = _map(P, S, K, seed)
    dev_in = {k: torch.tensor(v, device="cuda") for k, v in inp.items()}
    tilted, identity = torch.tensor(TILTED, device="cuda"), torch.eye(4, device="cuda")
    first = True
    for name, ts, step in _selections(P, seed + 1):
        mask = R.select_mask(ts, step)
        n = int(mask.sum())
        assert n == R.plan_counts(ts, max(step, 0) + 1)[step] if step >= 0 else n == 0
        ts_dev, mask_dev = torch.tensor(ts, device="cuda"), torch.tensor(mask, device="cuda")
        picked = {k: v[mask_dev].contiguous() for k, v in dev_in.items()}      # the reference's boolean index (:109)
        want_index = torch.nonzero(mask_dev).reshape(-1).to(torch.int32)
        for w2c_dev in (None, tilted):
            for rot_source in (ROT_PARAMS, ROT_TRANSFORMED):
                transform_rots = S == 3 and w2c_dev is not None
                what = (name, n, w2c_dev is not None, rot_source)
                oracle = _view_prep(picked, identity if w2c_dev is None else w2c_dev, S, transform_rots, rot_source)      # the view path's own kernel
                oracle["colors"] = picked["rgb_colors"]
                if w2c_dev is None:
                    oracle["means3D"] = picked["means3D"]
                got, index, count = _select(dev_in, ts_dev, step, S, K, transform_rots, rot_source, w2c_dev, n, n + 3)
                assert count == n, what
                for k, _c in OUTPUTS:
                    assert torch.equal(_bits(got[k][:n]), _bits(oracle[k])), (k, what)
                    assert (got[k][n:] == POISON).all(), (k, what)
                    if k in ("unnorm_rotations", "rotations", "opacities", "scales"):
                        assert torch.equal(got[k][:n], oracle[k]), (k, what)
                if K:
                    assert torch.equal(_bits(got["semantic"][:n]), _bits(picked["semantic"])), what
                    assert (got["semantic"][n:] == POISON).all(), what
                else:
                    assert (got["semantic"] == POISON).all(), what
                assert torch.equal(index[:n], want_index) and (index[n:] == POISON_INT).all(), what
                if n >= 1 and first:
                    # capacity = n - 1: row n - 1 of every output keeps its poison and the count is still n
                    less, index1, count1 = _select(dev_in, ts_dev, step, S, K, transform_rots, rot_source, w2c_dev, n - 1, n + 3)
                    assert count1 == n, what
                    for k in list(dict(OUTPUTS)) + (["semantic"] if K else []):
                        assert torch.equal(_bits(less[k][:n - 1]), _bits(got[k][:n - 1])) and (less[k][n - 1:] == POISON).all(), (k, what)
                    assert torch.equal(index1[:n - 1], want_index[:n - 1]) and (index1[n - 1:] == POISON_INT).all(), what
                    # the optional outputs may be NULL: the others are the same
                    some, index2, count2 = _select(dev_in, ts_dev, step, S, K, transform_rots, rot_source, w2c_dev, n, n + 3,
                                                   nulls=("unnorm_rotations", "semantic", "index"))
                    assert count2 == n and (index2 == POISON_INT).all() and (some["unnorm_rotations"] == POISON).all()
                    assert (some["semantic"] == POISON).all()
                    for k in ("means3D", "rotations", "opacities", "scales", "colors"):
                        assert torch.equal(_bits(some[k]), _bits(got[k])), (k, what)
                    # capacity = 0: only the count
                    none, _index3, count3 = _select(dev_in, ts_dev, step, S, K, transform_rots, rot_source, w2c_dev, 0, 4)
                    assert count3 == n and all((v == POISON).all() for v in none.values())
                    first = False


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("K", [0, 3, 26])
@pytest.mark.parametrize("P", [1, 255, 256, 257, 1023, 70001])
def test_select_equals_view_prep_on_the_indexed_rows_bit_for_bit(P, K, S):
    _check_selection(P, K, S, 100 * P + 10 * K + S)


@pytest.mark.parametrize("S", [1, 3])
def test_select_with_more_than_1024_block_counts(S):
    """300 007 rows are 1172 blocks: each thread of the one-workgroup scan owns more than one count"""
    _check_selection(300007, 26, S, 17 + S)


def test_select_of_an_empty_map():
    """P == 0: the count is written (0), nothing else"""
    empty = {k: torch.zeros((0, c), device="cuda") for k, c in (("means3D", 3), ("unnorm_rotations", 4), ("logit_opacities", 1),
                                                                ("log_scales", 1), ("rgb_colors", 3), ("semantic", 3))}
    ts = torch.zeros(1, device="cuda")      # never read
    got, index, count = _select(empty, ts, 3, 1, 3, False, ROT_PARAMS, None, 4, 4)
    assert count == 0 and (index == POISON_INT).all() and all((v == POISON).all() for v in got.values())


def test_replay_rendervars_is_one_select_sized_from_the_plan():
    from hsr_utils import replay, slam_helpers as SH
    P, K = 3000, 5
    for S in (1, 3):
        inp = _map(P, S, K, 40 + S)
        params = {k: torch.tensor(v, device="cuda") for k, v in inp.items()}
        ts = _timestep_vectors(P, 4, 9)["permuted"]
        plan = replay.ReplayPlan(torch.tensor(ts, device="cuda"), 4)
        for step in range(4):
            mask = torch.tensor(R.select_mask(ts, step), device="cuda")
            picked = {k: v[mask].contiguous() for k, v in params.items()}
            for semantic in (False, True):
                rv = replay.replay_rendervars(params, plan, step, semantic=semantic)
                keys = ["means3D", "colors_precomp", "rotations", "opacities", "scales"] + (["semantics_precomp"] if semantic else []) + ["means2D"]
                assert list(rv) == keys and all(v.shape[0] == plan.counts[step] for v in rv.values())
                assert torch.equal(_bits(rv["means3D"]), _bits(picked["means3D"])) and not rv["means2D"].any()
                assert rv["opacities"].shape == (plan.counts[step], 1) and rv["scales"].shape[1] == 3
                world = _view_prep(picked, torch.eye(4, device="cuda"), S, False, ROT_PARAMS if semantic else ROT_TRANSFORMED)
                for k in ("rotations", "opacities", "scales"):
                    assert torch.equal(rv[k].reshape(world[k].shape), world[k]), (k, step, semantic, S)
                assert torch.equal(_bits(rv["colors_precomp"]), _bits(picked["rgb_colors"]))
                assert not semantic or torch.equal(_bits(rv["semantics_precomp"]), _bits(picked["semantic"]))
                # in the camera frame: the rendervar of transform_to_view on the indexed map
                cam = replay.replay_rendervars(params, plan, step, semantic=semantic, w2c=TILTED)
                tg = SH.transform_to_view(picked, TILTED)
                want = (SH.transformed_params2rendervar_semantic if semantic else SH.transformed_params2rendervar)(picked, tg)
                for k in ("means3D", "rotations", "opacities", "scales", "colors_precomp") + (("semantics_precomp",) if semantic else ()):
                    assert torch.equal(_bits(cam[k]), _bits(want[k])), (k, step, semantic, S)


# ---- the point cloud ------------------------------------------------------------------------------------------------------------------------
def _cloud_case(H, W, seed):
    g = np.random.default_rng(seed)
    depth = (g.random((H, W)) * 5 + 0.3).astype(np.float32)
    flat = depth.reshape(-1)
    for i, v in enumerate((0.0, -1.25, np.inf, np.nan)[:max(0, flat.size - 1)]):
        flat[(i * 7) % flat.size if flat.size > 28 else i] = v
    picture = g.integers(0, 256, (H, W, 3)).astype(np.uint8)
    k = np.array([[57.3, 0, W / 2 - 0.37], [0, 61.1, H / 2 + 0.21], [0, 0, 1]], np.float32)
    return depth, picture, k


def _cloud(depth, picture, k, c2w_dev, odd):
    """hsr_replay_cloud through the C ABI, both outputs in one call; records at a 4-byte-aligned or at an odd address"""
    from diff_gaussian_rasterization import _abi
    dev = _device()
    H, W = depth.shape
    N = H * W
    depth_dev, picture_dev = torch.tensor(depth, device=dev), torch.tensor(picture, device=dev)
    points = torch.full((N * 3 + 16,), POISON, device=dev)
    raw = torch.full((N * 15 + 32,), 0xA5, dtype=torch.uint8, device=dev)
    assert raw.data_ptr() % 4 == 0
    off = 5 if odd else 4
    _abi.call(_abi.lib.hsr_replay_cloud, "hsr_replay_cloud", dev, H, W, depth_dev.data_ptr(), picture_dev.data_ptr(), float(k[0][0]), float(k[1][1]),
              float(k[0][2]), float(k[1][2]), c2w_dev.data_ptr(), points.data_ptr(), raw.data_ptr() + off)
    assert (points[N * 3:] == POISON).all() and (raw[:off] == 0xA5).all() and (raw[off + N * 15:] == 0xA5).all()
    return points[:N * 3].view(N, 3).cpu().numpy(), raw[off:off + N * 15].cpu().numpy()


def _same_records(got, want):
    """byte-equal, except that a NaN coordinate compares as 'is NaN' (the sign and payload of a NaN that an operation makes are the
    hardware's, not the chain's: the same rule as for the points)"""
    a, b = got.view(R.RECORD), want.view(R.RECORD)
    clean = ~(np.isnan(b["x"]) | np.isnan(b["y"]) | np.isnan(b["z"]))
    return (got.shape == want.shape and np.array_equal(got.reshape(-1, 15)[clean], want.reshape(-1, 15)[clean])
            and all(R.same_floats(a[c], b[c]) for c in "xyz") and all(np.array_equal(a[c], b[c]) for c in ("red", "green", "blue")))


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd address"])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (3, 4), (37, 53), (64, 96)])
def test_cloud_equals_the_float32_restatement_bit_for_bit(H, W, odd, tmp_path):
    """derivable, not measured: the file is built without contraction and every operation of the chain is one correctly rounded IEEE
    operation in a stated order, so the points are the restatement's bit for bit"""
    from hsr_utils import replay
    depth, picture, k = _cloud_case(H, W, 31 * H + W)
    w2c_dev = torch.tensor(TILTED, device="cuda")
    c2w_dev = torch.linalg.inv(w2c_dev).contiguous()      # as view_cloud forms it
    want_points = R.rgbd2pcd(depth, k, c2w_dev.cpu().numpy())
    want_records = R.records(want_points, picture)
    if H * W >= 5:
        flat = depth.reshape(-1)
        assert (flat == 0).any() and (flat < 0).any() and np.isinf(flat).any() and np.isnan(flat).any()
    points, recs = _cloud(depth, picture, k, c2w_dev, odd)
    assert R.same_floats(points, want_points), np.argwhere(points.view(np.uint32) != want_points.view(np.uint32))[:5]
    assert _same_records(recs, want_records)
    zero = np.argwhere(depth.reshape(-1) == 0).reshape(-1)
    if zero.size:      # zero depth lands on the camera centre
        assert np.array_equal(points[zero[0]], c2w_dev.cpu().numpy()[:3, 3])
    if odd:
        return
    # the Python layer: the same launch with one output each, and the file
    depth_dev, picture_dev = torch.tensor(depth, device="cuda")[None], torch.tensor(picture, device="cuda")
    p2 = replay.view_cloud(depth_dev, k, w2c_dev)
    r2 = replay.view_cloud(depth_dev, k, TILTED, picture=picture_dev, records=True)
    assert p2.shape == (H * W, 3) and np.array_equal(p2.cpu().numpy().view(np.uint32), points.view(np.uint32))
    assert r2.shape == (H * W, 15) and r2.dtype == torch.uint8 and np.array_equal(r2.cpu().numpy().reshape(-1), recs)
    path = replay.save_cloud_ply(str(tmp_path / "cloud.ply"), r2)
    data = open(path, "rb").read()
    header = data[:data.index(b"end_header\n") + len(b"end_header\n")]
    assert header == (b"ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                      b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % (H * W))
    assert len(data) == len(header) + 15 * H * W and data[len(header):] == recs.tobytes()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
W_, H_, K_, T_ = 96, 64, 26, 6


@pytest.fixture(scope="module")
def run():
    """a finished run in the shape of params.npz: about 5000 Gaussians, six poses, the timesteps 0..5 assigned non-monotonically"""
    from hsr_utils import make_scene
    from hsr_utils.camera import replica_intrinsics
    from test_gpu_slam_session import _gt_path
    P = 5003
    kmat = replica_intrinsics(W_, H_)
    sc = make_scene(P, W_, H_, K_, kmat, seed=11, kind="slam", scale_mult=2.0)
    rots, trans = _gt_path()
    g = torch.Generator().manual_seed(12)
    params = {"means3D": sc["means3D"], "rgb_colors": sc["colors_precomp"], "unnorm_rotations": sc["rotations"],
              "logit_opacities": torch.logit(sc["opacities"].clamp(1e-4, 1 - 1e-4)), "log_scales": sc["scales"][:, :1].log(),
              "semantic": sc["semantics_precomp"], "cam_unnorm_rots": rots, "cam_trans": trans,
              "timestep": torch.randint(0, T_, (P,), generator=g).float()}
    params = {k: v.float().contiguous().cuda() for k, v in params.items()}
    params.update(intrinsics=np.asarray(kmat, np.float32), w2c=np.eye(4, dtype=np.float32), org_width=W_, org_height=H_)
    return params, kmat


def _white(cam):
    return cam._replace(bg=torch.ones(3, device="cuda"))


def _render(rv, cam, semantic):
    from diff_gaussian_rasterization import GaussianRasterizer, GaussianRasterizer_semantic
    with torch.no_grad():
        if semantic:
            im, _radius, sem, depth, _median, opac = GaussianRasterizer_semantic(raster_settings=cam)(**rv)
            return im, depth, sem, opac
        im, _radius, depth, _median, opac, _mask = GaussianRasterizer(raster_settings=cam)(**rv)
        return im, depth, None, opac


@pytest.mark.parametrize("semantic", [False, True], ids=["plain", "semantic"])
def test_replay_view_equals_the_rasterizer_on_the_indexed_map(run, semantic):
    """the inputs are bit-equal and in equal order and the forward has no float atomics: the images are expected equal bit for bit"""
    from hsr_utils import replay, setup_camera, slam
    params, kmat = run
    ts = params["timestep"].cpu().numpy()
    assert (np.diff(ts) < 0).any() and set(ts.tolist()) == set(range(T_))
    plan = replay.ReplayPlan(params["timestep"], T_)
    w2cs = replay.run_w2cs(params)
    assert w2cs.is_cuda and all(torch.equal(w2cs[t], slam.frame_w2c(params, t)) for t in range(T_))
    first_view = w2cs[0].cpu().numpy().copy()
    first_view[:3, 3] += np.array([0, 0, 0.5], np.float32)
    identity = torch.eye(4, device="cuda")
    for t in range(T_):
        view = replay.follow_camera(first_view, w2cs[t].cpu().numpy())
        got = replay.replay_view(params, plan, t, view, kmat, W_, H_, semantic=semantic)
        mask = params["timestep"] <= t
        picked = {k: params[k][mask].contiguous() for k in ("means3D", "unnorm_rotations", "logit_opacities", "log_scales", "rgb_colors", "semantic")}
        n = int(mask.sum())
        assert n == plan.counts[t] and 0 < n
        o = _view_prep(picked, identity, 1, False, ROT_PARAMS if semantic else ROT_TRANSFORMED)
        rv = {"means3D": picked["means3D"], "colors_precomp": picked["rgb_colors"], "rotations": o["rotations"], "opacities": o["opacities"],
              "scales": o["scales"], "means2D": torch.zeros(n, 3, device="cuda")}
        if semantic:
            rv["semantics_precomp"] = picked["semantic"]
        cam = _white(setup_camera(W_, H_, kmat, view, device="cuda"))
        want = _render(rv, cam, semantic)
        again = _render(rv, cam, semantic)
        for a, b in zip(want, again):      # the oracle side alone: the forward is reproducible run to run
            assert a is None or torch.equal(a, b)
        for name, a, b in zip(("im", "depth", "im_semantic", "silhouette"), got, want):
            assert (a is None and b is None) or torch.equal(a, b), (name, t)
        assert got[0].shape == (3, H_, W_) and got[1].shape == (1, H_, W_) and (got[2] is None) == (not semantic)
        assert float(got[3].max()) > 0.5      # something is in view
    # at the last step the whole map shows: slam.render_view on a world-frame camera (the identity as the pose, the view in the camera)
    assert plan.counts[T_ - 1] == params["means3D"].shape[0]
    _rv, im, _radius, sem, depth, opac = slam.render_view(params, identity, cam, semantic)
    for a, b in zip(got, (im, depth, sem, opac)):
        assert (a is None and b is None) or torch.equal(a, b)


def _listing(folder):
    return {n: open(os.path.join(folder, n), "rb").read() for n in sorted(os.listdir(folder))}


def test_replay_run_writes_the_pictures_and_clouds_and_repeats_itself(run, tmp_path):
    from hsr_utils import replay
    from PIL import Image
    params, kmat = run
    written = replay.replay_run(params, str(tmp_path / "a"), every=2, cloud=True)
    assert written == [0, 2, 4]
    files = _listing(str(tmp_path / "a"))
    assert sorted(files) == sorted(["%d.png" % t for t in written] + ["%d.ply" % t for t in written])
    assert replay.replay_run(params, str(tmp_path / "b"), every=2, cloud=True) == written and _listing(str(tmp_path / "b")) == files
    plan = replay.ReplayPlan(params["timestep"], T_)
    w2cs = replay.run_w2cs(params).cpu().numpy()
    for t in written:
        picture = np.asarray(Image.open(str(tmp_path / "a" / ("%d.png" % t))))
        assert picture.shape == (H_, W_, 3) and picture.dtype == np.uint8
        im, depth, _sem, _sil = replay.replay_view(params, plan, t, w2cs[t], params["intrinsics"], W_, H_, semantic=False)      # float32, as saved
        assert np.array_equal(picture, np.rint(im.clamp(0, 1).permute(1, 2, 0).cpu().numpy() * np.float32(255)).astype(np.uint8))
        data = files["%d.ply" % t]
        body = np.frombuffer(data[data.index(b"end_header\n") + 11:], np.uint8)
        c2w = torch.linalg.inv(torch.tensor(w2cs[t], device="cuda")).cpu().numpy()
        assert b"element vertex %d\n" % (H_ * W_) in data and _same_records(body, R.records(R.rgbd2pcd(depth[0].cpu().numpy(), kmat, c2w), picture))
    # the last step alone, semantic rasterizer, depth pictures, a follow camera
    follow = w2cs[0].copy()
    follow[2, 3] += 0.5
    last = replay.replay_run(params, str(tmp_path / "c"), semantic=True, picture="depth", follow=follow, steps=[T_ - 1], depth_range=(0.0, 8.0))
    assert last == [T_ - 1] and sorted(os.listdir(str(tmp_path / "c"))) == ["%d.png" % (T_ - 1)]


def _tool():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "replay_run.py")
    spec = importlib.util.spec_from_file_location("replay_run_tool", path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_session_replay_and_the_tool_on_its_saved_map(sequence, tmp_path, monkeypatch, capsys):  # noqa: F811
    """a short session, its own replay(), then tools/replay_run.py on the params.npz it saves: one PNG per step"""
    import random
    import test_gpu_slam_session as TS
    from hsr_utils import SlamSession, map_io
    cam, intrinsics, frames = sequence
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    config = TS._config(2)
    config["mapping"]["num_iters"] = 2
    s = SlamSession(config, intrinsics, torch.eye(4, device="cuda"), cam)
    for frame in frames[:4]:
        s.step(frame)
    ts = s.variables["timestep"].cpu().numpy()
    assert set(ts.tolist()) <= {0.0, 1.0, 2.0, 3.0} and (ts == 0).any()
    assert s.replay(str(tmp_path / "session")) == [0, 1, 2, 3]
    assert sorted(os.listdir(str(tmp_path / "session"))) == ["%d.png" % t for t in range(4)]
    out = map_io.finalize_params(s.params, s.variables, intrinsics, torch.eye(4), TS.W, TS.H, [f["gt_w2c"] for f in frames[:4]],
                                 s.keyframe_time_indices)
    path = map_io.save_params(out, str(tmp_path / "run"))
    tool = _tool()
    monkeypatch.setattr(sys, "argv", ["replay_run.py", path, str(tmp_path / "tool"), "--cloud", "--semantic"])
    tool.main()
    assert "wrote %d steps" % TS.FRAMES in capsys.readouterr().out
    names = sorted(os.listdir(str(tmp_path / "tool")))
    assert names == sorted(["%d.png" % t for t in range(TS.FRAMES)] + ["%d.ply" % t for t in range(TS.FRAMES)])
    for t in range(4):      # the steps the session replayed: the same pictures, from the saved map
        assert open(str(tmp_path / "tool" / ("%d.png" % t)), "rb").read() == open(str(tmp_path / "session" / ("%d.png" % t)), "rb").read()
