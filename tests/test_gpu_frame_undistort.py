"""GPU suite for hsr_utils.frames.ingest_frame_undistort / hsr_frame_ingest_undistort (include/sensor/hsr_frame_undistort.h): every
output is compared BIT FOR BIT with the numpy restatement of the header, tests/undistort_ref.py (which tests/test_frame_undistort_cpu.py
shows to EQUAL an independent restatement on these cases), as tests/test_gpu_frame_ingest.py does with its restatement: colour and depth
as int32 words, labels as int64.  Depth and labels are not undistorted: they must equal ingest_frame's outputs on the same inputs.  Then
the route through SlamSession.ingest(undistort=...) and one step() on such a frame."""
import functools

import numpy as np
import pytest
import torch

import ingest_ref as I
import undistort_ref as U

pytestmark = pytest.mark.gpu

# the second and third level of the multi-level calls: one shrinks, one enlarges (tests/test_gpu_frame_ingest.py)
EXTRA = ((3, 5), (41, 29))
SCALE = 5000.0


@functools.lru_cache(maxsize=None)
def _frame(size):
    col, dep = I.make_frame(*size, seed=100 * size[0] + size[1])
    return col, dep, torch.from_numpy(col).cuda(), torch.from_numpy(dep.view(np.int16)).cuda()


@functools.lru_cache(maxsize=None)
def _reference(case, dst):
    size, camera, dist = U.CASES[case]
    col, dep, _c, _d = _frame(size)
    return U.color(col, dst, camera, dist), I.depth(dep, dst, SCALE)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check(got, want_color, want_depth):
    c, d = got
    assert c.dtype == d.dtype == torch.float32 and c.is_contiguous() and d.is_contiguous()
    assert tuple(c.shape) == want_color.shape and tuple(d.shape) == (1,) + want_depth.shape
    differ = _bits(c.cpu().numpy()) != _bits(want_color)
    assert not differ.any(), "%d of %d colour values differ from the restatement" % (int(differ.sum()), differ.size)
    assert np.array_equal(_bits(d.cpu().numpy()[0]), _bits(want_depth))


@pytest.mark.parametrize("n_levels", [1, 2, 3])
@pytest.mark.parametrize("case", U.SMALL_CASES)
def test_levels_match_the_restatement_bit_for_bit(case, n_levels):
    from hsr_utils import ingest_frame_undistort
    size, camera, dist = U.CASES[case]
    _col, _dep, col_d, dep_d = _frame(size)
    sizes = [size] + list(EXTRA[:n_levels - 1])
    levels, labels = ingest_frame_undistort(col_d, dep_d, sizes, SCALE, camera, dist)
    assert labels is None and len(levels) == n_levels
    for dst, got in zip(sizes, levels):
        _check(got, *_reference(case, dst))
    again, _ = ingest_frame_undistort(col_d, dep_d, sizes, SCALE, camera, dist)      # two calls are bit-identical
    for a, b in zip(again, levels):
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


@pytest.mark.parametrize("case", ["23x37-fr1", "23x37-outside"])
def test_a_reduced_and_an_enlarged_level_0(case):
    """level 0 is not the sensor's size: every level takes the four-tap path (and the sensor-sized one, last, the one-tap path)"""
    from hsr_utils import ingest_frame_undistort
    size, camera, dist = U.CASES[case]
    _col, _dep, col_d, dep_d = _frame(size)
    for sizes in ([EXTRA[0], EXTRA[1], size], [(12, 19)], [(46, 74), (22, 37)]):
        levels, _ = ingest_frame_undistort(col_d, dep_d, sizes, SCALE, camera, dist)
        for dst, got in zip(sizes, levels):
            _check(got, *_reference(case, dst))


def test_tum_fr1_frame_to_itself():
    from hsr_utils import ingest_frame_undistort
    size, camera, dist = U.CASES["480x640-fr1"]
    _col, _dep, col_d, dep_d = _frame(size)
    (got,), _ = ingest_frame_undistort(col_d, dep_d, [size], SCALE, camera, dist)
    want_color, want_depth = _reference("480x640-fr1", size)
    _check(got, want_color, want_depth)
    assert not want_color[:, 0, 0].any() and not want_color[:, -1, -1].any() and want_color[:, 240, 320].any()      # the black border
    # four coefficients: k3 = 0
    (got4,), _ = ingest_frame_undistort(col_d, dep_d, [size], SCALE, camera, dist[:4])
    col = _frame(size)[0]
    assert np.array_equal(_bits(got4[0].cpu().numpy()), _bits(U.color(col, size, camera, dist[:4] + (0.0,))))


def _label_case(size, seed=5):
    g = np.random.default_rng(seed)
    ids = g.integers(-2, 16, size=size).astype(np.int32)      # the table knows 0..11
    table = g.integers(-1, 40, size=(12, 3)).astype(np.int32)
    table[3] = -1
    return ids, table


@pytest.mark.parametrize("kind", ["uint16", "int32", "float32"])
def test_depth_and_labels_are_the_plain_ingests(kind):
    """not undistorted: depth in the three types and labels with a 3-level table equal ingest_frame's outputs bit for bit on the same
    inputs (and the restatement), while the colour is the undistorted one"""
    from hsr_utils import ingest_frame, ingest_frame_undistort
    case = "23x37-fr1"
    size, camera, dist = U.CASES[case]
    sizes = [(12, 19), size, EXTRA[1]]
    col, dep16, col_d, _d = _frame(size)
    if kind == "uint16":
        raw = dep16.copy()
        raw[1, :4] = (0, 65535, 32768, 32767)
        given = raw
    elif kind == "int32":
        raw = dep16.astype(np.int32) * 30000
        raw[1, :4] = (0, 2 ** 31 - 1, -5, 65536)
        given = torch.from_numpy(raw).cuda()
    else:
        raw = dep16.astype(np.float32) * np.float32(0.37)
        raw[1, :5] = (np.nan, np.inf, 0.0, -np.inf, 1e-30)
        given = torch.from_numpy(raw)
    ids, table = _label_case(size)
    table_d = torch.from_numpy(table).cuda()
    levels, labels = ingest_frame_undistort(col_d, given, sizes, SCALE, camera, dist, labels=ids, tree_table=table_d)
    plain, plain_labels = ingest_frame(col_d, given, sizes, SCALE, labels=ids, tree_table=table_d)
    assert labels.dtype == torch.int64 and torch.equal(labels, plain_labels)
    assert np.array_equal(labels.cpu().numpy(), I.labels(ids, sizes[0], table))
    for dst, (c, d), (pc, pd) in zip(sizes, levels, plain):
        assert torch.equal(d.view(torch.int32), pd.view(torch.int32)), (kind, dst)      # NaN payloads included: the same instructions
        want = I.depth(raw, dst, SCALE)
        nan = np.isnan(want)
        got = d.cpu().numpy()[0]
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])
        assert np.array_equal(_bits(c.cpu().numpy()), _bits(_reference(case, dst)[0]))
        assert not torch.equal(c, pc)


@pytest.mark.parametrize("size", [(23, 37), (48, 64)], ids=["23x37", "48x64"])
def test_zero_coefficients_equal_the_plain_ingest(size):
    from hsr_utils import ingest_frame, ingest_frame_undistort
    _col, _dep, col_d, dep_d = _frame(size)
    camera = U.SMALL_CAMERA if size == (23, 37) else (53.54, 53.92, 32.01, 24.76)
    sizes = [size, (size[0] // 2, size[1] // 2), EXTRA[1]]
    levels, _ = ingest_frame_undistort(col_d, dep_d, sizes, SCALE, camera, (0.0, 0.0, 0.0, 0.0))
    plain, _ = ingest_frame(col_d, dep_d, sizes, SCALE)
    for (c, d), (pc, pd) in zip(levels, plain):
        assert torch.equal(c.view(torch.int32), pc.view(torch.int32)) and torch.equal(d.view(torch.int32), pd.view(torch.int32))


@pytest.mark.parametrize("lens", [((20.0, 21.0, 6.0, 4.0), (1e200,) * 5), ((20.0, 21.0, 6.0, 4.0), (1e200, -1e200, 1e200, -1e200, 1e200)), U.OVERFLOW],
                         ids=["1e200", "1e200-signs", "overflow"])
def test_huge_coefficients_leave_the_principal_point_alone(lens):
    """far outside, inf and NaN coordinates: 0 everywhere except the principal point's pixel, at the sensor's size and at a reduced one"""
    from hsr_utils import ingest_frame_undistort
    camera, dist = lens
    col, dep = I.make_frame(9, 13, seed=2)
    col[4, 6] = (200, 100, 50)
    sizes = [(9, 13), (5, 7)]
    levels, _ = ingest_frame_undistort(col, dep, sizes, SCALE, camera, dist)
    full = levels[0][0].cpu().numpy()
    want = np.zeros((3, 9, 13), dtype=np.float32)
    want[:, 4, 6] = np.array([200, 100, 50], dtype=np.float32) / np.float32(255)
    assert np.array_equal(_bits(full), _bits(want))
    for dst, (c, _d) in zip(sizes, levels):
        assert np.array_equal(_bits(c.cpu().numpy()), _bits(U.color(col, dst, camera, dist)))


def test_host_and_non_contiguous_inputs_agree():
    from hsr_utils import ingest_frame_undistort
    case = "23x37-inside"
    size, camera, dist = U.CASES[case]
    sizes = [size, (12, 19)]
    col, dep, col_d, dep_d = _frame(size)
    ids, table = _label_case(size)
    table_d = torch.from_numpy(table).cuda()
    a, la = ingest_frame_undistort(col, dep, sizes, SCALE, camera, np.asarray(dist), labels=ids, tree_table=table_d)       # numpy
    b, lb = ingest_frame_undistort(torch.from_numpy(col), torch.from_numpy(dep.view(np.int16)), sizes, SCALE, list(camera), torch.tensor(dist),
                                   labels=torch.from_numpy(ids), tree_table=torch.from_numpy(table))                        # host tensors
    wide = torch.zeros((size[0], 2 * size[1], 3), dtype=torch.uint8, device="cuda")
    wide[:, ::2] = col_d
    assert not wide[:, ::2].is_contiguous()
    c, lc = ingest_frame_undistort(wide[:, ::2], dep_d, sizes, SCALE, camera, dist, labels=torch.from_numpy(ids).cuda(), tree_table=table_d)
    for other, lo in ((b, lb), (c, lc)):
        assert torch.equal(la, lo)
        for (c0, d0), (c1, d1) in zip(a, other):
            assert torch.equal(c0.view(torch.int32), c1.view(torch.int32)) and torch.equal(d0.view(torch.int32), d1.view(torch.int32))
    for dst, got in zip(sizes, a):
        _check(got, *_reference(case, dst))


def test_one_launch_and_refusals_launch_nothing(monkeypatch):
    from hsr_utils import frames, ingest_frame_undistort
    calls, plain = [], []
    real = frames._lib.hsr_frame_ingest_undistort
    monkeypatch.setattr(frames._lib, "hsr_frame_ingest_undistort", lambda *a: calls.append(a) or real(*a))
    monkeypatch.setattr(frames._lib, "hsr_frame_ingest", lambda *a: plain.append(a))
    size, camera, dist = U.CASES["23x37-fr1"]
    _col, _dep, col_d, dep_d = _frame(size)
    with pytest.raises(ValueError, match="thin-prism"):
        ingest_frame_undistort(col_d, dep_d, [size], SCALE, camera, dist + (0.0,))
    with pytest.raises(ValueError, match="fx and fy"):
        ingest_frame_undistort(col_d, dep_d, [size], SCALE, (0.0, 1.0, 1.0, 1.0), dist)
    with pytest.raises(ValueError, match="ingest_frame"):
        ingest_frame_undistort(col_d, dep_d, [size] * 4, SCALE, camera, dist)
    assert calls == []
    ingest_frame_undistort(col_d, dep_d, [size, EXTRA[0], EXTRA[1]], SCALE, camera, dist)
    assert len(calls) == 1 and plain == []      # three levels, one launch, of this entry


def test_invalid_arguments_write_nothing():
    """the C entry point itself with device pointers: a zero fx, a NaN coefficient, a side of 16385 — each an error code, and the
    sentinel-filled outputs unchanged; the same call with valid arguments writes"""
    from diff_gaussian_rasterization import _abi
    size, camera, dist = U.CASES["23x37-fr1"]
    _col, _dep, col_d, dep_d = _frame(size)
    fill = -7.25
    out_c, out_d = torch.full((3 * 24,), fill, device="cuda"), torch.full((24,), fill, device="cuda")

    def call(Ws=size[1], camera=camera, dist=dist):
        arr = (_abi.hsr_ingest_level * 1)(_abi.hsr_ingest_level(4, 6, out_c.data_ptr(), out_d.data_ptr()))
        with torch.cuda.device(col_d.device):
            rc = _abi.lib.hsr_frame_ingest_undistort(size[0], Ws, col_d.data_ptr(), dep_d.data_ptr(), 0, SCALE, None, 0, None, 0, *camera, *dist,
                                                     1, arr, None, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, _abi.lib.hsr_last_error()
    for kw, message in ((dict(camera=(0.0,) + camera[1:]), b"fx and fy"), (dict(dist=dist[:4] + (float("nan"),)), b"coefficients"),
                        (dict(Ws=16385), b"sides")):
        rc, err = call(**kw)
        assert rc == -1 and err.startswith(b"frame_ingest_undistort:") and message in err, (kw, rc, err)
        assert bool((out_c == fill).all()) and bool((out_d == fill).all()), kw
    rc, _err = call()
    assert rc == 0 and not bool((out_c == fill).any()) and not bool((out_d == fill).any())


# ---- through the session --------------------------------------------------------------------------------------------------------------
SH_, SW_ = 48, 64
LENS = (61.0, 60.5, 31.2, 24.3, (0.2624, -0.9531, -0.0054, 0.0026, 1.1633))
TREE = {0: (0, 0), "1": (0, 1), 2: (1, 0), 3: (1, 1)}


def _sensor_frame():
    """a smooth colour image, a smooth depth map around 2.5 m in units of 1/5000 m, class ids 0..3 in quadrants"""
    v, u = np.mgrid[0:SH_, 0:SW_].astype(np.float64)
    col = np.stack([127 + 100 * np.sin(u / 7.0), 127 + 100 * np.cos(v / 5.0), 127 + 100 * np.sin((u + v) / 9.0)], axis=-1).astype(np.uint8)
    dep = ((2.5 + 0.3 * np.sin(u / 15.0) + 0.2 * np.cos(v / 11.0)) * SCALE).astype(np.uint16)
    ids = (2 * (u > SW_ / 2) + (v > SH_ / 2)).astype(np.uint8)
    return col, dep, ids


def _session(sizes):
    import test_gpu_slam_session_multires as M
    from hsr_utils import SlamSession, setup_camera
    kmat = [[LENS[0], 0.0, LENS[2]], [0.0, LENS[1], LENS[3]], [0.0, 0.0, 1.0]]
    cam = setup_camera(SW_, SH_, kmat, np.eye(4), device="cuda")
    cfg = M._config(3, sizes=sizes)
    cfg["data"]["num_frames"] = 2
    cfg["data"]["png_depth_scale"] = SCALE
    return SlamSession(cfg, torch.tensor(kmat, dtype=torch.float32, device="cuda"), torch.eye(4, device="cuda"), cam)


def test_session_ingest_undistort_and_one_step():
    from hsr_utils import ingest_frame_undistort, tree_label_table
    col, dep, ids = _sensor_frame()
    table = tree_label_table(TREE, 2, device="cuda")
    reduced = (SH_ // 2, SW_ // 2)
    s = _session((reduced, reduced))
    frame = s.ingest(0, col, dep, gt_w2c=torch.eye(4, device="cuda"), labels=ids, tree_table=table, undistort=LENS)
    assert set(frame) == {"id", "im", "depth", "gt_w2c", "semantic_label_gt", "tracking_im", "tracking_depth", "densify_im", "densify_depth"}
    levels, labels = ingest_frame_undistort(col, dep, [(SH_, SW_), reduced], SCALE, LENS[:4], LENS[4], labels=ids, tree_table=table)
    for got, want in ((frame["im"], levels[0][0]), (frame["depth"], levels[0][1]), (frame["tracking_im"], levels[1][0]),
                      (frame["tracking_depth"], levels[1][1])):
        assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert frame["densify_im"] is frame["tracking_im"] and frame["densify_depth"] is frame["tracking_depth"]
    assert torch.equal(frame["semantic_label_gt"], labels) and tuple(labels.shape) == (3, SH_, SW_)
    assert np.array_equal(_bits(frame["im"].cpu().numpy()), _bits(U.color(col, (SH_, SW_), LENS[:4], LENS[4])))
    assert np.array_equal(_bits(frame["tracking_im"].cpu().numpy()), _bits(U.color(col, reduced, LENS[:4], LENS[4])))
    s.step(frame)
    torch.cuda.synchronize()
    assert len(s.keyframe_list) == 1 and s.keyframe_list[0]["color"] is frame["im"]
    assert int(s.params["means3D"].shape[0]) > 0 and bool(torch.isfinite(s.params["means3D"]).all())
    # a session without reduced sizes: the frame's own keys only
    plain = _session(None).ingest(0, col, dep, labels=ids, tree_table=table, undistort=LENS)
    assert set(plain) == {"id", "im", "depth", "semantic_label_gt"} and torch.equal(plain["im"].view(torch.int32), frame["im"].view(torch.int32))


def test_session_refuses_the_planes_combination():
    from hsr_utils import composed_label_table
    col, dep, ids = _sensor_frame()
    s = _session(None)
    table = composed_label_table(None, TREE, 2, device="cuda")
    with pytest.raises(ValueError, match="does not combine with the planes route"):
        s.ingest(0, col, dep, labels=ids, tree_table=table, leaf_column=True, undistort=LENS)
    with pytest.raises(ValueError, match="does not combine with the planes route"):
        s.ingest(0, col, dep[::2, ::2], undistort=LENS)
    with pytest.raises(ValueError, match="does not combine with the planes route"):
        s.ingest(0, col, dep, labels=np.zeros((96, 128), np.uint8), undistort=LENS)
