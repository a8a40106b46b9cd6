"""CPU suite for the depth image of a mesh (include/recon/hsr_mesh_depth.h, hsr_utils.mesh_depth): the header through the helpers of
tests/test_abi.py (its prototypes, that the library exports them and that _abi.RECON_HEADERS binds them with the header's types); every
refusal of the header with dummy pointers; the scratch size; the lazy names; the numpy restatement (tests/mesh_depth_ref.py) against the
same formulas in float64 on the tilted-plane scene; virtual_views against the construction its docstring states; the host errors of
hsr_utils.mesh_depth.  Nothing here launches: there is no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_depth_ref as R
import test_abi

HEADER = "recon/hsr_mesh_depth.h"
NAMES = ["hsr_mesh_depth_scratch_bytes", "hsr_mesh_depth"]
FP, VP, IP = ("pointer", "float"), ("pointer", "void"), ("pointer", "int")
NAN, INF = float("nan"), float("inf")


def test_mesh_depth_abi_exported_and_bound():
    from diff_gaussian_rasterization import _abi
    protos = test_abi._prototypes([HEADER])
    assert list(_abi.RECON_HEADERS) == [HEADER] and HEADER not in _abi.HEADERS and HEADER not in _abi.EVAL_HEADERS
    assert HEADER not in test_abi.ALL_HEADERS
    assert [s[0] for s in _abi.RECON_HEADERS[HEADER]] == list(protos) == NAMES      # the header's names in the header's order
    assert test_abi.check_header(HEADER) == NAMES      # exported, and bound with the header's type classes
    for name, restype, argtypes in _abi.RECON_HEADERS[HEADER]:      # _load() bound this table as it binds the other two
        fn = getattr(_abi.lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    bound = [s[0] for tables in (_abi.HEADERS, _abi.EVAL_HEADERS, _abi.RECON_HEADERS) for table in tables.values() for s in table]
    assert sorted(bound) == sorted(set(bound))      # no name twice across the three tables
    assert protos["hsr_mesh_depth_scratch_bytes"][1:] == ("size_t", ["int", "int", "int"])
    assert protos["hsr_mesh_depth"][1:] == ("int", ["int", "int", FP, IP, "int", "int"] + ["float"] * 4 + [FP, "float", VP, "size_t", FP, IP, VP])
    assert _abi.lib.hsr_mesh_depth.argtypes[10] is _abi.fp      # w2c is the one HOST pointer: a ctypes array goes in by address
    from hsr_utils import mesh_depth, mesh_eval
    source = test_abi._source(HEADER)
    for name, value in (("HSR_MESH_MAX_IMAGE_SIDE", mesh_eval.MAX_IMAGE_SIDE), ("HSR_MESH_DEPTH_SMALL_BOX", mesh_depth.SMALL_BOX)):
        assert "#define %s %d\n" % (name, value) in source
    assert "#define HSR_MESH_MAX_IMAGE_SIDE %d\n" % mesh_eval.MAX_IMAGE_SIDE in test_abi._source("eval/hsr_mesh_eval.h")      # one value, stated twice
    assert mesh_depth.SMALL_BOX == R.SMALL_BOX >= 16      # the smallest box of a face inside the image is 3 x 3, the usual one 4 x 4


def test_names_are_reached_lazily_from_the_package():
    import hsr_utils
    from hsr_utils import mesh_depth, mesh_eval
    assert tuple(hsr_utils._MESH_DEPTH) == tuple(mesh_depth.__all__)
    for name in hsr_utils._MESH_DEPTH:
        assert getattr(hsr_utils, name) is getattr(mesh_depth, name), name
    assert not set(hsr_utils._MESH_DEPTH) & (set(hsr_utils._MESH_EVAL) | set(hsr_utils._MESH))
    assert tuple(hsr_utils._MESH_EVAL) == tuple(mesh_eval.__all__)
    import inspect
    keywords = inspect.signature(mesh_eval.evaluate_mesh_run).parameters
    assert [keywords[n].default for n in ("depth_views", "depth_seed", "depth_size")] == [0, 0, None]


# ---- refusals: dummy non-device pointers that are never followed ---------------------------------------------------------------------------
W2C = (C.c_float * 16)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1)
D = [4096 * (n + 1) for n in range(8)]      # 16-byte aligned


def depth_call(lib, V=4, F=2, vertices=D[0], faces=D[1], H=6, W=8, fx=8.0, fy=8.0, cx=3.5, cy=2.5, w2c=W2C, near=0.01, scratch=D[2],
               scratch_bytes=None, out_depth=D[3], out_face=D[4]):
    if scratch_bytes is None:
        scratch_bytes = lib.hsr_mesh_depth_scratch_bytes(max(F, 0), max(H, 0), max(W, 0))
    return lib.hsr_mesh_depth(V, F, vertices, faces, H, W, fx, fy, cx, cy, w2c, near, scratch, scratch_bytes, out_depth, out_face, None)


REFUSALS = (
    [(o, b"invalid sizes") for o in (dict(V=0), dict(V=-2), dict(F=-1))]
    + [(o, b"invalid image size") for o in (dict(H=0), dict(W=0), dict(H=16385), dict(W=16385), dict(H=-4))]
    + [(dict(near=v), b"near must be finite and positive") for v in (0.0, -0.01, NAN, INF, -INF)]
    + [({n: v}, b"must be finite and not zero") for n in ("fx", "fy") for v in (0.0, NAN, INF, -INF)]
    + [({n: v}, b"cx and cy finite") for n in ("cx", "cy") for v in (NAN, INF)]
    + [({n: None}, b"are required") for n in ("w2c", "out_depth", "out_face", "scratch")]
    + [({n: None}, b"are required with F > 0") for n in ("vertices", "faces")]
    + [(dict(scratch_bytes=0), b"the scratch must hold"), (dict(scratch_bytes=6 * 8 * 8 + 16 + 16 - 1), b"the scratch must hold")]
    + [(dict(scratch=D[2] + 8), b"16-byte aligned"), (dict(scratch=D[2] + 4), b"16-byte aligned")]
)


@pytest.mark.parametrize("overrides,message", REFUSALS, ids=["%d" % i for i in range(len(REFUSALS))])
def test_entry_point_refuses_before_any_device_work(overrides, message):
    from diff_gaussian_rasterization import _abi
    rc = depth_call(_abi.lib, **overrides)
    err = _abi.lib.hsr_last_error()
    assert rc == -1 and err.startswith(b"mesh_depth: ") and message in err, (overrides, rc, err)


def test_scratch_bytes_is_monotone_and_positive():
    from diff_gaussian_rasterization import _abi
    size = _abi.lib.hsr_mesh_depth_scratch_bytes
    assert size(0, 1, 1) > 0 and size(0, 6, 8) >= 6 * 8 * 8
    assert size(2, 6, 8) == 6 * 8 * 8 + 16 + 16      # the key image, the list of two faces rounded up to 16 bytes, the counter's 16
    by_faces = [size(F, 48, 64) for F in (0, 1, 3, 4, 5, 1000, 10 ** 6, 2 ** 31 - 1)]
    assert by_faces == sorted(by_faces) and by_faces[0] < by_faces[3] < by_faces[4] < by_faces[-1] and all(b % 16 == 0 for b in by_faces)
    assert by_faces[-2] >= 48 * 64 * 8 + 4 * 10 ** 6 + 4
    by_pixels = [size(100, H, W) for H, W in ((1, 1), (1, 2), (2, 2), (13, 17), (48, 64), (680, 1200), (16384, 16384))]
    assert by_pixels == sorted(by_pixels) and len(set(by_pixels[1:])) == len(by_pixels) - 1      # one and two pixels both take 16 bytes
    assert by_pixels[-1] >= 8 * 16384 * 16384      # past 2^31: the size is a size_t


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def test_restatement_against_float64_on_the_tilted_plane():
    """The float32 rule against the same formulas in float64 on the same float32 inputs: 128 jittered faces of one plane, every winding
    and rotation.  Measured on this scene (seed 0): the largest relative depth error is 2.87e-6 (1.9e-6 against the analytic plane; seeds
    1..3 of the generator give 2.1e-6, 6.6e-6 and 3.3e-6); four times the scene's own figure is allowed.  3 of the 3055 hit pixels have a
    float64 barycentric weight within 1e-4 of zero and are left out of the face comparison (the cap is 5 %)."""
    vertices, faces = R.tilted_plane(0)
    assert faces.shape == (128, 3) and vertices.dtype == np.float32
    depth, face = R.render(vertices, faces, np.eye(4), R.PLANE_K, R.PLANE_H, R.PLANE_W)
    depth64, face64, margin = R.render64(vertices, faces, np.eye(4), R.PLANE_K, R.PLANE_H, R.PLANE_W)
    assert depth.dtype == np.float32 and face.dtype == np.int32 and depth.shape == face.shape == (48, 64)
    hit, hit64 = face >= 0, face64 >= 0
    truth, inner = R.plane_truth()
    assert inner.sum() == 3012 and hit[inner].all()      # every pixel whose ray meets the plane inside the inner region is hit: no hole
    assert np.array_equal(depth == 0, ~hit) and (depth[hit] > 0).all()
    both = hit & hit64
    assert both.sum() >= 3000 and (hit ^ hit64).sum() <= 0.01 * both.sum()      # the two outlines differ at most where a weight is ~0
    rel = np.abs(depth[both].astype(np.float64) - depth64[both]) / depth64[both]
    print("largest relative depth error against float64: %.3e; against the plane: %.3e" %
          (rel.max(), (np.abs(depth[inner] - truth[inner]) / truth[inner]).max()))
    assert rel.max() <= 4 * 2.87e-6
    assert (np.abs(depth[inner] - truth[inner]) / truth[inner]).max() <= 4 * 2.87e-6      # the vertices are rounded, the plane is not
    sure = both & (np.abs(margin) > 1e-4)
    left_out = int((both & ~sure).sum())
    print("left out of the face comparison: %d of %d" % (left_out, both.sum()))
    assert left_out <= 0.05 * both.sum()
    assert np.array_equal(face[sure], face64[sure])
    assert len(np.unique(face[hit])) > 60      # the image is made of many faces, not of one


def general_cameras():
    import scenes
    return scenes.CAMERAS


@pytest.mark.parametrize("camera", ["skew23", "skew140", "roll90", "pitch17"])
def test_restatement_against_float64_under_general_cameras(camera):
    """The identity and a turn about y leave m01, m10, m12, m21 of camera_points at 0 and m11 at 1.  The plane scene placed with the inverse
    of each general camera (every entry of the rotation live) and rendered through that camera: the float32 rule against float64 on the same
    float32 inputs, by the criteria of the test above.  Measured (largest relative depth error; pixels left out of the face comparison):
    skew23 1.6e-6, 3; skew140 3.2e-6, 3; roll90 2.8e-6, 3; pitch17 2.7e-6, 3 — within four times the identity scene's 2.87e-6, which holds unchanged."""
    w2c = general_cameras()[camera]
    vertices, faces = R.tilted_plane(0)
    world = R.place(vertices, w2c)
    assert np.abs(R.camera_points(world, w2c, np.float64) - vertices).max() < 5e-6      # back where they were, to the rounding of the placement
    depth, face = R.render(world, faces, w2c, R.PLANE_K, R.PLANE_H, R.PLANE_W)
    depth64, face64, margin = R.render64(world, faces, w2c, R.PLANE_K, R.PLANE_H, R.PLANE_W)
    hit, hit64 = face >= 0, face64 >= 0
    truth, inner = R.plane_truth()
    assert hit[inner].all()      # no hole
    both = hit & hit64
    assert both.sum() >= 3000 and (hit ^ hit64).sum() <= 0.01 * both.sum()
    rel = np.abs(depth[both].astype(np.float64) - depth64[both]) / depth64[both]
    sure = both & (np.abs(margin) > 1e-4)
    print("%s: largest relative depth error against float64 %.3e; left out of the face comparison %d of %d" % (camera, rel.max(), (both & ~sure).sum(), both.sum()))
    assert rel.max() <= 4 * 2.87e-6
    assert (np.abs(depth[inner] - truth[inner]) / truth[inner]).max() <= 4 * 2.87e-6
    assert (both & ~sure).sum() <= 0.05 * both.sum() and np.array_equal(face[sure], face64[sure])
    assert len(np.unique(face[hit])) > 60


@pytest.mark.parametrize("camera", ["skew23", "skew140", "roll90", "pitch17"])
def test_random_faces_scene_takes_both_paths_under_every_camera(camera):
    """the scene tests/test_gpu_mesh_depth.py renders under the general cameras holds what it is meant to: boxes on both sides of SMALL_BOX,
    faces across the camera's plane (whole-image boxes), both windings, and an image made of many faces"""
    w2c = general_cameras()[camera]
    k, H, W = R.PLANE_K, R.PLANE_H, R.PLANE_W
    vertices, faces = R.random_faces(3, k, H, W)
    boxes = []
    depth, face = R.render(R.place(vertices, w2c), faces, w2c, k, H, W, boxes=boxes)
    boxes = np.array(boxes)
    assert (boxes == 0).sum() > 0 and ((boxes > 0) & (boxes <= R.SMALL_BOX)).sum() > 40 and ((boxes > R.SMALL_BOX) & (boxes < H * W)).sum() > 20
    assert (boxes == H * W).sum() >= 2
    assert len(np.unique(face[face >= 0])) > 40 and (face >= 0).mean() > 0.5


def test_restatement_edges():
    k = np.array([[8.0, 0, 3.5], [0, 8.0, 2.5], [0, 0, 1]])
    v = np.array([[-1, -1, 2], [1, -1, 2], [0, 1, 2], [0, 0, NAN], [INF, 0, 2]], np.float32)
    one = R.render(v, np.array([[0, 1, 2]], np.int32), np.eye(4), k, 6, 8)
    assert (one[0][one[1] == 0] == 2).all() and 0 < (one[1] == 0).sum() < 48 and set(one[1].ravel().tolist()) == {0, -1}
    other = R.render(v, np.array([[0, 2, 1]], np.int32), np.eye(4), k, 6, 8)      # the other winding: the same image
    assert np.array_equal(one[0], other[0]) and np.array_equal(one[1], other[1])
    for bad in ([0, 1, 5], [-1, 1, 2], [0, 1, 3], [0, 1, 4], [0, 1, 1]):      # an index of V, of -1, a NaN, an infinity, det == 0
        boxes = []
        got = R.render(v, np.array([bad, [0, 1, 2]], np.int32), np.eye(4), k, 6, 8, boxes=boxes)
        assert boxes[0] == 0 and np.array_equal(got[0], one[0]) and np.array_equal(got[1], np.where(one[1] == 0, 1, -1))
    twice = R.render(v, np.array([[0, 1, 2], [0, 2, 1]], np.int32), np.eye(4), k, 6, 8)      # equal depths: the smaller index
    assert np.array_equal(twice[1], one[1])
    boxes = []
    behind = R.render(v * np.float32([1, 1, -1]), np.array([[0, 1, 2]], np.int32), np.eye(4), k, 6, 8, boxes=boxes)
    assert boxes == [0] and (behind[1] == -1).all() and (behind[0] == 0).all()      # wholly behind the camera: it takes no part
    boxes = []
    across = R.render(v * np.float32([1, 1, 1]) - np.float32([[0, 0, 0], [0, 0, 0], [0, 0, 2.5], [0, 0, 0], [0, 0, 0]]), np.array([[0, 1, 2]], np.int32),
                      np.eye(4), k, 6, 8, boxes=boxes)
    assert boxes == [48] and (across[1] == 0).sum() > 0 and (across[0][across[1] == 0] >= 0.01).all()      # one corner behind: tested at every pixel
    empty = R.render(v, np.zeros((0, 3), np.int32), np.eye(4), k, 6, 8)
    assert (empty[1] == -1).all() and (empty[0] == 0).all()


# ---- virtual views ------------------------------------------------------------------------------------------------------------------------
def view_fixture():
    """two poses and six targets: the first target is the first pose's centre and the second lies straight along its image-down axis"""
    a = np.eye(4)
    a[:3, 3] = [0.2, -0.1, 0.5]
    c, s = np.cos(0.7), np.sin(0.7)
    b = np.eye(4)
    b[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.array([[1, 0, 0], [0, np.cos(0.3), -np.sin(0.3)], [0, np.sin(0.3), np.cos(0.3)]])
    b[:3, 3] = [-1.0, 0.3, 2.0]
    poses = np.stack([a, b])
    centre = -a[:3, :3].T @ a[:3, 3]
    targets = np.concatenate([[centre], [centre + 2 * a[1, :3]], np.random.default_rng(1).uniform(-3, 3, (4, 3)) + [0, 0, 4]])
    return poses, targets


def test_virtual_views_follow_the_stated_construction():
    from hsr_utils import mesh_depth
    poses, targets = view_fixture()
    n, seed = 24, 17
    views = mesh_depth.virtual_views(poses, targets, n, seed=seed)
    assert isinstance(views, np.ndarray) and views.dtype == np.float32 and views.shape == (n, 4, 4)
    assert np.array_equal(views, mesh_depth.virtual_views(torch.tensor(poses), torch.tensor(targets), n, seed=seed))      # the same for the same seed
    assert not np.array_equal(views, mesh_depth.virtual_views(poses, targets, n, seed=seed + 1))
    assert np.array_equal(views[:5], mesh_depth.virtual_views(poses, targets, 5, seed=seed))      # view i does not depend on n
    assert mesh_depth.virtual_views(poses, targets, 0).shape == (0, 4, 4)
    assert mesh_depth._splitmix(0, 1) == R.splitmix(0, 1) == 0xE220A8397B1DCDAF
    cases = [R.view_case(poses, targets, i, seed) for i in range(n)]
    assert cases.count("pose") == 1 and cases.count("fallback") == 1      # each special case occurs, once
    for i, view in enumerate(views.astype(np.float64)):
        a, b = R.view_choice(len(poses), len(targets), i, seed)
        pose = poses[a]
        rot = view[:3, :3]
        assert np.array_equal(view[3], [0, 0, 0, 1])
        assert np.abs(rot @ rot.T - np.eye(3)).max() <= 1e-6 and abs(np.linalg.det(rot) - 1) <= 1e-6
        centre, want_centre = -rot.T @ view[:3, 3], -pose[:3, :3].T @ pose[:3, 3]
        assert np.abs(centre - want_centre).max() <= 1e-5      # it stands where the pose stood
        if cases[i] == "pose":
            assert np.array_equal(views[i], pose.astype(np.float32))
            continue
        p = rot @ targets[b] + view[:3, 3]      # the target lies on the axis: it projects to the principal point
        assert p[2] > 0 and abs(600.0 * p[0] / p[2]) <= 1e-2 and abs(600.0 * p[1] / p[2]) <= 1e-2
        if cases[i] == "down":      # the pose's image-down axis, made perpendicular to the new viewing axis, is the new image-down axis
            assert abs(rot[0] @ pose[1, :3]) <= 1e-6 and rot[1] @ pose[1, :3] > 0
        else:                        # the pose's image-right axis takes that part for the new image-right axis
            assert abs(rot[1] @ pose[0, :3]) <= 1e-6 and rot[0] @ pose[0, :3] > 0
            assert np.linalg.norm(np.cross(rot[2], pose[1, :3])) < 1e-3


# ---- the host side -------------------------------------------------------------------------------------------------------------------------
def test_host_errors():
    from hsr_utils import mesh_depth
    v, f = torch.zeros(3, 3), torch.zeros((1, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="vertices must be a tensor on a HIP device; there is no CPU path"):
        mesh_depth.MeshDepthRenderer(v, f, 4, 4)
    with pytest.raises(RuntimeError, match="vertices must be a tensor on a HIP device; there is no CPU path"):
        mesh_depth.render_mesh_depth(v.numpy(), f.numpy(), np.eye(4), np.eye(3), 4, 4)
    with pytest.raises(RuntimeError, match="vertices of rec or gt must be a tensor on a HIP device; there is no CPU path"):
        mesh_depth.mesh_depth_l1((v, f), (v, f), np.eye(4)[None], np.eye(3), 4, 4)
    for H, W in ((0, 4), (4, 0), (16385, 4)):
        with pytest.raises(ValueError, match="the image is %d x %d" % (W, H)):
            mesh_depth.MeshDepthRenderer(v, f, H, W)
    with pytest.raises(RuntimeError, match=r"w2cs must be \[T,4,4\]"):
        mesh_depth.mesh_depth_l1((v, f), (v, f), np.eye(4), np.eye(3), 4, 4)
    with pytest.raises(RuntimeError, match=r"w2cs must be \[T,4,4\] with T >= 1"):
        mesh_depth.virtual_views(np.zeros((0, 4, 4)), np.zeros((2, 3)), 3)
    with pytest.raises(RuntimeError, match=r"targets must be \[M,3\] with M >= 1"):
        mesh_depth.virtual_views(np.eye(4)[None], np.zeros((0, 3)), 3)
    with pytest.raises(RuntimeError, match=r"targets must be \[M,3\]"):
        mesh_depth.virtual_views(np.eye(4)[None], np.zeros(3), 3)
    with pytest.raises(ValueError, match="number of views must be >= 0"):
        mesh_depth.virtual_views(np.eye(4)[None], np.zeros((2, 3)), -1)
