"""CPU suite for the ingest that undistorts the colour image (include/sensor/hsr_frame_undistort.h, hsr_utils.frames.ingest_frame_undistort,
SlamSession.ingest(undistort=...)) and for the TUM RGB-D reader (hsr_utils.sequence.TUMSequence): the header through the helpers of
tests/test_abi.py (its prototype, that the library exports it and that _abi.SENSOR_HEADERS binds it with the header's types); every
refusal of the header with fake pointers; the numpy restatement of the header (tests/undistort_ref.py) against an independent one, with
no pixel excluded; the sign of the map, zero and huge coefficients; the reader on a directory the test writes; the argument errors of
the Python entries that need no device.  Nothing here launches: there is no GPU."""
import os

import numpy as np
import pytest
import torch

import ingest_ref as I
import test_abi
import undistort_ref as U

HEADER = "sensor/hsr_frame_undistort.h"
NAME = "hsr_frame_ingest_undistort"
NAN, INF = float("nan"), float("inf")


def test_frame_undistort_abi_exported_and_bound():
    from diff_gaussian_rasterization import _abi
    protos = test_abi._prototypes([HEADER])
    assert list(_abi.SENSOR_HEADERS) == [HEADER] and HEADER not in test_abi.ALL_HEADERS
    assert all(HEADER not in table for table in (_abi.HEADERS, _abi.EVAL_HEADERS, _abi.RECON_HEADERS))
    assert [s[0] for s in _abi.SENSOR_HEADERS[HEADER]] == list(protos) == [NAME]
    assert test_abi.check_header(HEADER) == [NAME]      # exported, and bound with the header's type classes
    for name, restype, argtypes in _abi.SENSOR_HEADERS[HEADER]:      # _load() bound this table as it binds the other three
        fn = getattr(_abi.lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    bound = [s[0] for tables in (_abi.HEADERS, _abi.EVAL_HEADERS, _abi.RECON_HEADERS, _abi.SENSOR_HEADERS) for table in tables.values()
             for s in table]
    assert sorted(bound) == sorted(set(bound))      # no name twice across the four tables
    vp = ("pointer", "void")
    # hsr_frame_ingest's parameters with nine doubles between n_ids and n_out
    plain = test_abi._prototypes(["ext/hsr_frame_ingest.h"])["hsr_frame_ingest"]
    assert protos[NAME][1] == plain[1] == "int"
    assert protos[NAME][2] == plain[2][:10] + ["double"] * 9 + plain[2][10:]
    assert protos[NAME][2][20] == ("pointer", "hsr_ingest_level") and protos[NAME][2][22] == vp
    assert test_abi._structures([HEADER]) == {}      # it reuses hsr_ingest_level


def _call(lib, **kw):
    """hsr_frame_ingest_undistort with fake pointers that are never followed: every call made with this is refused before the launch"""
    from diff_gaussian_rasterization import _abi
    fake = 4096
    a = dict(Hs=8, Ws=8, color=fake, depth=fake, depth_type=0, scale=5000.0, labels=None, L=0, table=None, n_ids=0,
             fx=517.3, fy=516.5, cx=318.6, cy=255.3, k1=0.2624, k2=-0.9531, p1=-0.0054, p2=0.0026, k3=1.1633,
             n_out=1, sizes=((4, 4),), outs=(fake, fake), out_labels=None, levels="array")
    a.update(kw)
    arr = (_abi.hsr_ingest_level * 4)(*[_abi.hsr_ingest_level(h, w, a["outs"][0], a["outs"][1]) for h, w in (tuple(a["sizes"]) + ((4, 4),) * 4)[:4]])
    return lib.hsr_frame_ingest_undistort(a["Hs"], a["Ws"], a["color"], a["depth"], a["depth_type"], a["scale"], a["labels"], a["L"], a["table"],
                                          a["n_ids"], a["fx"], a["fy"], a["cx"], a["cy"], a["k1"], a["k2"], a["p1"], a["p2"], a["k3"], a["n_out"],
                                          arr if a["levels"] == "array" else None, a["out_labels"], None)


def test_frame_undistort_refuses_before_any_device_work():
    """everything hsr_frame_ingest refuses (the cases of tests/test_frame_ingest_cpu.py), under this entry's name, and the camera and the
    coefficients: an error code and a message, not a launch (no pointer here is a device pointer)"""
    from diff_gaussian_rasterization import _abi
    lib, fake = _abi.lib, 4096
    for kw in (dict(Hs=0), dict(Ws=16385), dict(Hs=-2), dict(sizes=((0, 4),)), dict(sizes=((4, 16385),)),
               dict(n_out=2, sizes=((4, 4), (16385, 4))), dict(n_out=3, sizes=((4, 4), (4, 4), (4, 0)))):
        assert _call(lib, **kw) == -1 and b"frame_ingest_undistort: sides" in lib.hsr_last_error(), kw
    for kw in (dict(n_out=0), dict(n_out=4), dict(n_out=-1), dict(levels=None)):
        assert _call(lib, **kw) == -1 and b"frame_ingest_undistort: n_out" in lib.hsr_last_error(), kw
    for kw in (dict(depth_type=3), dict(depth_type=-1)):
        assert _call(lib, **kw) == -1 and b"frame_ingest_undistort: depth_type" in lib.hsr_last_error(), kw
    for kw in (dict(scale=0.0), dict(scale=-0.0), dict(scale=INF), dict(scale=NAN)):
        assert _call(lib, **kw) == -1 and b"frame_ingest_undistort: depth_scale" in lib.hsr_last_error(), kw
    for kw in (dict(L=-1), dict(L=17, table=fake, n_ids=4), dict(L=2, labels=fake, out_labels=fake),
               dict(L=2, table=fake, n_ids=0, labels=fake, out_labels=fake)):
        assert _call(lib, **kw) == -1 and b"frame_ingest_undistort: num_levels" in lib.hsr_last_error(), kw
    for kw in (dict(color=None), dict(depth=None), dict(outs=(None, fake)), dict(outs=(fake, None)), dict(labels=fake), dict(out_labels=fake),
               dict(Hs=16384, Ws=16384, color=None, n_out=3, sizes=((16384, 16384), (1, 16384), (16384, 1)))):
        assert _call(lib, **kw) == -1 and b"frame_ingest_undistort: NULL" in lib.hsr_last_error(), kw
    for name in ("fx", "fy"):
        for bad in (0.0, -0.0, INF, -INF, NAN):
            assert _call(lib, **{name: bad}) == -1 and b"frame_ingest_undistort: fx and fy" in lib.hsr_last_error(), (name, bad)
    for name in ("cx", "cy", "k1", "k2", "p1", "p2", "k3"):
        for bad in (INF, -INF, NAN):
            assert _call(lib, **{name: bad}) == -1 and b"frame_ingest_undistort: cx, cy and the coefficients" in lib.hsr_last_error(), (name, bad)
    # the other entries keep their own names
    assert lib.hsr_frame_ingest(0, 8, fake, fake, 0, 1.0, None, 0, None, 0, 1, None, None, None) == -1
    assert lib.hsr_last_error().startswith(b"frame_ingest: n_out")


# ---- the two restatements against each other -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(U.CASES))
def test_restatements_agree_with_no_pixel_excluded(case):
    """the header's order in numpy against other expressions of the coordinates in torch and scipy's map_coordinates: EQUAL.  U is an
    exact integer over 1024 in both, so the two can differ only where a coordinate quantises to another 1/32 step, and two associations
    of the coordinates (which differ by a few ulp of ~640 * 32, 1e-11) can do that only where 32 * us or 32 * vs lies within 1e-9 of a
    half-integer.  Such pixels may be excluded, and only those; on these cases none is."""
    (Hs, Ws), camera, dist = U.CASES[case]
    col, _dep = I.make_frame(Hs, Ws, seed=31 * Hs + Ws)
    us, vs = U.source(Hs, Ws, camera, dist)
    sx, ax, nanx = U.steps(us)
    sy, ay, nany = U.steps(vs)
    (iu, inanx), (iv, inany) = (U.independent_steps(c) for c in U.independent_source(Hs, Ws, camera, dist))
    assert not nanx.any() and not nany.any() and not inanx.any() and not inany.any()
    differ = (sx * 32 + ax != iu) | (sy * 32 + ay != iv)
    excluded = differ & (U.near_half(us) | U.near_half(vs))
    print("%s: %d quantised coordinates differ, %d pixels excluded" % (case, int(differ.sum()), int(excluded.sum())))
    assert np.array_equal(differ, excluded)      # a differing step anywhere else is an error of one of the two
    assert not excluded.any()                    # and on the listed cases there is none
    mine, other = U.undistorted(col, camera, dist), U.independent_undistorted(col, camera, dist)
    assert mine.dtype == other.dtype == np.float64 and mine.shape == other.shape == (3, Hs, Ws)
    assert np.array_equal(mine, other)
    assert np.array_equal(mine * 1024.0, np.round(mine * 1024.0)) and mine.min() >= 0.0 and mine.max() <= 255.0
    # what the cases are there for
    outside = (sx < -1) | (sx >= Ws) | (sy < -1) | (sy >= Hs)
    partly = ((sx < 0) | (sx + 1 >= Ws) | (sy < 0) | (sy + 1 >= Hs)) & ~outside
    assert not mine[:, outside].any()
    if case == "480x640-fr1":
        assert 15000 <= outside.sum() <= 17000 and 1500 <= partly.sum() <= 2500
    if case == "23x37-outside":
        assert (int(outside.sum()), int(partly.sum())) == (250, 70)
    if case == "23x37-inside":
        assert not outside.any() and not partly.any() and np.abs(us - np.arange(Ws)[None, :]).max() > 2.5


def test_sign_of_the_map_at_the_corners():
    """k1 < 0 (barrel): the source of every corner pixel lies nearer the principal point than the pixel; k1 > 0: farther"""
    (Hs, Ws), camera = (480, 640), U.FR1[0]
    corners = [(0, 0), (0, Ws - 1), (Hs - 1, 0), (Hs - 1, Ws - 1)]
    for k1, nearer in ((-0.2, True), (0.2, False)):
        us, vs = U.source(Hs, Ws, camera, (k1, 0.0, 0.0, 0.0, 0.0))
        for v, u in corners:
            pixel = np.hypot(u - camera[2], v - camera[3])
            src = np.hypot(us[v, u] - camera[2], vs[v, u] - camera[3])
            assert (src < pixel - 5.0) if nearer else (src > pixel + 5.0), (k1, v, u, src, pixel)


@pytest.mark.parametrize("size", [(480, 640), (23, 37), (1, 1)], ids=["480x640", "23x37", "1x1"])
def test_zero_coefficients_give_the_plain_ingest_bit_for_bit(size):
    (Hs, Ws) = size
    camera = (535.4, 539.2, 320.1, 247.6) if size == (480, 640) else U.SMALL_CAMERA      # TUM fr3
    col, _dep = I.make_frame(Hs, Ws, seed=5)
    zero = (0.0,) * 5
    us, vs = U.source(Hs, Ws, camera, zero)
    assert np.abs(us - np.arange(Ws)[None, :]).max() <= 3e-14 and np.abs(vs - np.arange(Hs)[:, None]).max() <= 3e-14
    assert np.array_equal(U.undistorted(col, camera, zero), col.transpose(2, 0, 1).astype(np.float64))
    for dst in {size, (max(1, Hs // 2), max(1, Ws // 2)), (41, 29)}:
        assert np.array_equal(U.color(col, dst, camera, zero).view(np.int32), I.color(col, dst).view(np.int32)), dst


def test_huge_coefficients_leave_the_principal_point_alone():
    """coefficients of 1e200 with integer cx, cy: every coordinate but the principal point's is far outside, so the image is 0
    everywhere except that pixel, which keeps its value; with 1e300 and a focal length of 1e-3 the polynomial overflows, and the
    coordinates are inf, or inf - inf or 0 * inf, a NaN: still 0"""
    Hs, Ws, camera = 9, 13, (20.0, 21.0, 6.0, 4.0)
    col, _dep = I.make_frame(Hs, Ws, seed=2)
    col[4, 6] = (200, 100, 50)
    for dist in ((1e200,) * 5, (1e200, -1e200, 1e200, -1e200, 1e200), (-1e200,) * 5):
        got = U.undistorted(col, camera, dist)
        want = np.zeros((3, Hs, Ws))
        want[:, 4, 6] = (200, 100, 50)
        assert np.array_equal(got, want), dist
    us, vs = U.source(Hs, Ws, camera, (1e200,) * 5)
    assert np.isfinite(us).all() and np.abs(np.delete(us.reshape(-1), 4 * Ws + 6)).min() > 1e190 and us[4, 6] == 6.0 and vs[4, 6] == 4.0
    us, vs = U.source(Hs, Ws, U.OVERFLOW[0], U.OVERFLOW[1])
    assert np.isnan(us).any() and np.isinf(us).any() and np.isnan(vs).any() and us[4, 6] == 6.0 and vs[4, 6] == 4.0
    assert np.array_equal(U.undistorted(col, *U.OVERFLOW), want)
    sx, ax, nan = U.steps(np.array([np.nan, np.inf, -np.inf, 1e300, -33.0 / 32, -0.5 / 32, 0.5 / 32, 1.5 / 32]))
    assert nan.tolist() == [True] + [False] * 7
    assert sx[1:].tolist() == [2 ** 25, -2 ** 25, 2 ** 25, -2, 0, 0, 0] and ax[1:].tolist() == [0, 0, 0, 31, 0, 0, 2]      # half to even


# ---- the TUM reader ------------------------------------------------------------------------------------------------------------------
TUM_H, TUM_W = 6, 8
# colour timestamps: 1.00 kept; 1.02 closer than 1/32 s to it: thinned; 1.10 kept; 2.00 has no depth within max_dt; 3.00 kept;
# 3.04 kept (more than 1/32 s after 3.00)
T_COLOR = (1.00, 1.02, 1.10, 2.00, 3.00, 3.04)
T_DEPTH = (1.01, 1.11, 2.50, 2.99, 3.05)
T_POSE = (0.99, 1.03, 1.12, 2.01, 3.01, 3.03, 9.0)
KEPT = ((0, 0, 0), (2, 1, 2), (4, 3, 4), (5, 4, 5))      # (colour line, depth line, pose line)


def _pose_cells(k):
    """tx ty tz qx qy qz qw of pose line k: the quaternion is NOT normalised (norms 0.5 .. 3.5)"""
    g = np.random.default_rng(100 + k)
    q = g.normal(size=4)
    q *= (0.5 + 0.5 * k) / np.linalg.norm(q)
    return np.concatenate([g.normal(size=3), q])


@pytest.fixture(scope="module", params=["groundtruth.txt", "pose.txt"])
def tum_dir(request, tmp_path_factory):
    from PIL import Image
    base = tmp_path_factory.mktemp("tum")
    seq = base / "freiburg9_desk"
    (seq / "rgb").mkdir(parents=True)
    (seq / "depth").mkdir()
    g = np.random.default_rng(8)
    colors, depths = [], []
    with open(seq / "rgb.txt", "w") as f:
        f.write("# color images\n# file: 'x.bag'\n# timestamp filename\n")
        for t in T_COLOR:
            col = g.integers(0, 256, size=(TUM_H, TUM_W, 3), dtype=np.uint8)
            Image.fromarray(col).save(seq / "rgb" / ("%.6f.png" % t))
            f.write("%.6f rgb/%.6f.png\n" % (t, t))
            colors.append(col)
    with open(seq / "depth.txt", "w") as f:
        f.write("# depth maps\n")
        for t in T_DEPTH:
            dep = g.integers(0, 65536, size=(TUM_H, TUM_W)).astype(np.uint16)
            Image.fromarray(dep).save(seq / "depth" / ("%.6f.png" % t))
            f.write("%.6f depth/%.6f.png\n" % (t, t))
            depths.append(dep)
    with open(seq / request.param, "w") as f:
        f.write("# ground truth trajectory\n# timestamp tx ty tz qx qy qz qw\n")
        for k, t in enumerate(T_POSE):
            f.write("%.4f %s\n" % (t, " ".join(repr(float(v)) for v in _pose_cells(k))))
            if k == 2:
                f.write("# a comment between the poses\n\n")
    return str(base), colors, depths


def _c2w(k):
    from scipy.spatial.transform import Rotation
    cells = _pose_cells(k)
    m = np.eye(4)
    m[:3, :3] = Rotation.from_quat(cells[3:]).as_matrix()      # scalar last; scipy normalises
    m[:3, 3] = cells[:3]
    return m


def test_tum_sequence_association_thinning_and_poses(tum_dir):
    from hsr_utils import TUMSequence
    from hsr_utils.sequence import quaternion_c2w
    base, colors, depths = tum_dir
    seq = TUMSequence(base, "freiburg9_desk")
    assert len(seq) == 4 and seq.retained_inds == [0, 1, 2, 3] and [tuple(a) for a in seq.associations] == list(KEPT)
    assert seq.timestamps == [T_COLOR[i] for i, _j, _k in KEPT]
    assert os.path.basename(seq.pose_path) in ("groundtruth.txt", "pose.txt")
    first_inv = np.linalg.inv(_c2w(KEPT[0][2]))
    for n, (i, j, k) in enumerate(KEPT):
        color, depth, labels, gt_w2c = seq[n]
        assert color.dtype == np.uint8 and color.flags["C_CONTIGUOUS"] and np.array_equal(color, colors[i])
        assert depth.dtype == np.uint16 and np.array_equal(depth, depths[j]) and labels is None
        # the quaternion is not normalised: against scipy's Rotation, which normalises (a few float64 roundings of entries <= 1)
        assert np.abs(quaternion_c2w(_pose_cells(k)) - _c2w(k)).max() <= 1e-14
        want = np.linalg.inv(first_inv @ _c2w(k))
        assert gt_w2c.dtype == np.float32 and gt_w2c.shape == (4, 4) and np.abs(gt_w2c - want).max() <= 1e-6
    assert np.abs(seq[0][3] - np.eye(4)).max() <= 1e-7 and np.abs(seq[1][3] - np.eye(4)).max() > 0.05
    rot = quaternion_c2w(_pose_cells(3))[:3, :3]
    assert np.abs(rot @ rot.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(rot) - 1.0) <= 1e-14
    with pytest.raises(IndexError):
        seq[4]
    assert len(list(seq)) == 4
    # a wider max_dt takes the colour frame at 2.00 in (its nearest depth, 2.50, is 0.5 s away); a lower frame rate thins more
    assert [a[0] for a in TUMSequence(base, "freiburg9_desk", max_dt=0.6).associations] == [0, 2, 3, 4, 5]
    assert [a[0] for a in TUMSequence(base, "freiburg9_desk", frame_rate=5).associations] == [0, 4]
    assert [a[0] for a in TUMSequence(base, "freiburg9_desk", frame_rate=1000).associations] == [0, 1, 2, 4, 5]


def test_tum_sequence_start_end_stride_and_errors(tum_dir):
    from hsr_utils import TUMSequence
    base, colors, depths = tum_dir
    seq = TUMSequence(base, "freiburg9_desk", start=1, end=-1, stride=2)
    assert seq.retained_inds == [1, 3] and [tuple(a) for a in seq.associations] == [KEPT[1], KEPT[3]]
    assert np.abs(seq[0][3] - np.eye(4)).max() <= 1e-7      # relative to the first RETAINED frame
    want = np.linalg.inv(np.linalg.inv(_c2w(KEPT[1][2])) @ _c2w(KEPT[3][2]))
    assert np.abs(seq[1][3] - want).max() <= 1e-6 and np.array_equal(seq[1][1], depths[KEPT[3][1]])
    assert TUMSequence(base, "freiburg9_desk", start=0, end=3).retained_inds == [0, 1, 2]
    assert TUMSequence(base, "freiburg9_desk", start=2, end=3, stride=5).retained_inds == [2]
    for kw in (dict(start=-1), dict(start=2, end=2), dict(start=2, end=1), dict(stride=0)):
        with pytest.raises(ValueError, match="hsr_utils.sequence"):
            TUMSequence(base, "freiburg9_desk", **kw)
    with pytest.raises(RuntimeError, match="no frame"):
        TUMSequence(base, "freiburg9_desk", start=7)
    with pytest.raises(RuntimeError, match="rgb.txt"):
        TUMSequence(base, "nowhere")
    with pytest.raises(RuntimeError, match="within"):
        TUMSequence(base, "freiburg9_desk", max_dt=1e-4)


# ---- argument errors that need no device ---------------------------------------------------------------------------------------------
def test_ingest_frame_undistort_argument_errors():
    import hsr_utils
    from hsr_utils import frames, ingest_frame_undistort
    assert ingest_frame_undistort is frames.ingest_frame_undistort and "ingest_frame_undistort" in frames.__all__
    assert "TUMSequence" in hsr_utils._SEQUENCE
    col, dep = I.make_frame(4, 6)
    camera, dist = U.SMALL_CAMERA, U.FR1[1]
    with pytest.raises(ValueError, match="rational .* thin-prism"):
        ingest_frame_undistort(col, dep, [(4, 6)], 5000.0, camera, dist + (0.1,))
    with pytest.raises(ValueError, match="rational .* thin-prism"):
        ingest_frame_undistort(col, dep, [(4, 6)], 5000.0, camera, np.zeros(8))
    for bad in ((), (0.1,), (0.1, 0.2, 0.3)):
        with pytest.raises(ValueError, match="4 or 5 distortion coefficients"):
            ingest_frame_undistort(col, dep, [(4, 6)], 5000.0, camera, bad)
    for bad in ((1.0, 1.0, 1.0), (1.0,) * 5, 3.0):
        with pytest.raises(ValueError, match=r"camera must be \(fx, fy, cx, cy\)"):
            ingest_frame_undistort(col, dep, [(4, 6)], 5000.0, bad, dist)
    for bad in ((0.0, 1.0, 1.0, 1.0), (1.0, INF, 1.0, 1.0), (NAN, 1.0, 1.0, 1.0)):
        with pytest.raises(ValueError, match="fx and fy"):
            ingest_frame_undistort(col, dep, [(4, 6)], 5000.0, bad, dist)
    with pytest.raises(ValueError, match="must be finite"):
        ingest_frame_undistort(col, dep, [(4, 6)], 5000.0, (1.0, 1.0, NAN, 1.0), dist)
    with pytest.raises(ValueError, match="must be finite"):
        ingest_frame_undistort(col, dep, [(4, 6)], 5000.0, camera, (0.1, INF, 0.0, 0.0))
    # everything else is ingest_frame's to refuse
    with pytest.raises(RuntimeError, match="color_u8 must be"):
        ingest_frame_undistort(col[..., :2], dep, [(4, 6)], 5000.0, camera, dist)
    with pytest.raises(ValueError, match="png_depth_scale"):
        ingest_frame_undistort(col, dep, [(4, 6)], 0.0, camera, dist)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            ingest_frame_undistort(col, dep, [(4, 6)], 5000.0, camera, dist[:4])


def test_session_ingest_undistort_routes_and_refuses(monkeypatch):
    from hsr_utils import frames, slam

    class Cam:
        image_height, image_width = 4, 6
    lrs = dict(means3D=0.0, rgb_colors=0.0, unnorm_rotations=0.0, logit_opacities=0.0, log_scales=0.0, cam_unnorm_rots=4e-4, cam_trans=2e-3)
    config = dict(map_every=1, keyframe_every=3, mapping_window_size=4, data=dict(num_frames=8, png_depth_scale=5000.0),
                  tracking=dict(num_iters=5, lrs=lrs, loss_weights=dict(im=0.5, depth=1.0), sil_thres=0.99),
                  mapping=dict(num_iters=5, lrs=lrs, loss_weights=dict(im=0.5, depth=1.0), sil_thres=0.5))
    col, dep = I.make_frame(4, 6)
    seen = []

    def fake(color_u8, depth_raw, sizes, scale, camera, distortion, labels=None, tree_table=None):
        seen.append((list(sizes), scale, tuple(camera), tuple(distortion), labels is not None))
        out = [(torch.zeros(3, h, w), torch.zeros(1, h, w)) for h, w in sizes]
        return out, (None if labels is None else torch.zeros((1,) + tuple(sizes[0]), dtype=torch.int64))
    monkeypatch.setattr(frames, "ingest_frame_undistort", fake)
    monkeypatch.setattr(frames, "ingest_frame", lambda *a, **k: pytest.fail("the plain entry was called"))
    s = slam.SlamSession(config, torch.eye(3), torch.eye(4), cam=Cam())
    und = U.FR1[0] + (U.FR1[1],)
    frame = s.ingest(3, col, dep, undistort=und)
    assert seen == [([(4, 6)], 5000.0, U.FR1[0], U.FR1[1], False)] and set(frame) == {"id", "im", "depth"} and frame["id"] == 3
    frame = s.ingest(0, col, dep, labels=np.zeros((4, 6), np.uint8), gt_w2c=np.eye(4, dtype=np.float32), undistort=und)
    assert seen[-1][4] and set(frame) == {"id", "im", "depth", "gt_w2c", "semantic_label_gt"}
    for kw in (dict(leaf_column=True), dict(labels=np.zeros((8, 12), np.uint8))):
        with pytest.raises(ValueError, match="does not combine with the planes route"):
            s.ingest(0, col, dep, undistort=und, **kw)
    with pytest.raises(ValueError, match="does not combine with the planes route"):
        s.ingest(0, col, dep[:2, :3], undistort=und)
    for bad in ((1.0, 2.0, 3.0, 4.0), 5.0):
        with pytest.raises(ValueError, match="undistort must be"):
            s.ingest(0, col, dep, undistort=bad)
    assert len(seen) == 2
