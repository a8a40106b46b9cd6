"""GPU suite for the depth image of a mesh (include/recon/hsr_mesh_depth.h, hsr_utils.mesh_depth): every image against the numpy
restatement of tests/mesh_depth_ref.py — the depths bit for bit, the face images equal — at the smallest sizes at which the kernels can go
wrong: both windings, odd image sides, faces across and behind the camera's plane, equal depths, faces that take no part, both paths of
the split at its threshold, a list of large faces longer than the sweep's grid; Depth L1 on meshes whose answer is known; and the number
through the session, the module and the tool on the short session of tests/test_gpu_mesh_eval.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_depth_ref as R
import test_gpu_slam_session as TS
from test_gpu_mesh_eval import EVERY, SCORE, VOXEL, sequence, session  # noqa: F401  (the fixtures: six rendered frames and the short session)

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN, INF = float("nan"), float("inf")
EYE = np.eye(4)
K16 = np.array([[8.0, 0, 7.5], [0, 8.0, 5.5], [0, 0, 1]])          # 16 x 12; a power of two, so that rx and ry are exact
K64 = np.array([[32.0, 0, 31.5], [0, 32.0, 23.5], [0, 0, 1]])      # 64 x 48
TRIANGLE = np.array([[-1.5, -1.0, 2], [1.5, -1.0, 2], [0, 1.0, 2]], np.float32)


def dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(dtype)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def device_render(vertices, faces, w2c, k, H, W, near=0.01):
    from hsr_utils import mesh_depth
    depth, face = mesh_depth.render_mesh_depth(dev(vertices, torch.float32), dev(np.asarray(faces).reshape(-1, 3), torch.int32), w2c, k, H, W, near)
    assert depth.dtype == torch.float32 and face.dtype == torch.int32 and depth.shape == face.shape == (H, W) and depth.is_cuda
    return depth.cpu().numpy(), face.cpu().numpy()


def check(vertices, faces, w2c, k, H, W, near=0.01, boxes=None):
    """the device's image equals the restatement's: depths bit for bit, faces equal; returns (depth, face)"""
    want = R.render(vertices, faces, w2c, k, H, W, near, boxes=boxes)
    got = device_render(vertices, faces, w2c, k, H, W, near)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
    return got


# ---- one face -----------------------------------------------------------------------------------------------------------------------------
def test_one_triangle_and_its_other_winding():
    depth, face = check(TRIANGLE, [[0, 1, 2]], EYE, K16, 12, 16)
    assert 20 < (face == 0).sum() < 16 * 12 and (depth[face == 0] == 2).all() and (depth[face < 0] == 0).all()
    other = check(TRIANGLE, [[0, 2, 1]], EYE, K16, 12, 16)
    assert np.array_equal(bits(other[0]), bits(depth)) and np.array_equal(other[1], face)
    tilted = TRIANGLE + np.float32([[0, 0, 0.5], [0, 0, -0.25], [0, 0, 1.0]])      # depths that are not all one number
    a, b = check(tilted, [[0, 1, 2]], EYE, K16, 12, 16), check(tilted, [[1, 2, 0]], EYE, K16, 12, 16)
    assert np.array_equal(a[1], b[1]) and len(np.unique(a[0])) > 10


def test_odd_image_sides_and_one_pixel():
    import scenes
    k = np.array([[9.0, 0, 8.0], [0, 7.0, 6.0], [0, 0, 1]])
    vertices, faces = R.tilted_plane(1)
    depth, face = check(vertices, faces, scenes.tilted_w2c(), k, 13, 17)
    assert (face >= 0).sum() > 50
    one = check(TRIANGLE, [[0, 1, 2]], EYE, np.array([[8.0, 0, 0], [0, 8.0, 0], [0, 0, 1]]), 1, 1)
    assert one[0].tolist() == [[2.0]] and one[1].tolist() == [[0]]
    miss = check(TRIANGLE + np.float32([9, 0, 0]), [[0, 1, 2]], EYE, np.array([[8.0, 0, 0], [0, 8.0, 0], [0, 0, 1]]), 1, 1)
    assert miss[0].tolist() == [[0.0]] and miss[1].tolist() == [[-1]]


def test_faces_across_behind_and_at_the_near_plane():
    across = np.array([[-1.5, -1.0, 2], [1.5, -1.0, 2], [0, 0.5, -0.5]], np.float32)      # one corner behind the camera
    boxes = []
    depth, face = check(across, [[0, 1, 2]], EYE, K16, 12, 16, boxes=boxes)
    assert boxes == [16 * 12] and 0 < (face == 0).sum() < 16 * 12 and (depth[face == 0] >= 0.01).all()
    near = check(across, [[0, 1, 2]], EYE, K16, 12, 16, near=1.0)      # the same face, cut where its own depth passes 1
    assert 0 < (near[1] == 0).sum() < (face == 0).sum() and (near[0][near[1] == 0] >= 1.0).all()
    boxes = []
    behind = check(TRIANGLE * np.float32([1, 1, -1]), [[0, 1, 2]], EYE, K16, 12, 16, boxes=boxes)
    assert boxes == [0] and (behind[1] == -1).all() and (behind[0] == 0).all()      # wholly behind: it takes no part
    boxes = []
    check(TRIANGLE, [[0, 1, 2]], EYE, K16, 12, 16, near=np.nextafter(np.float32(2), np.float32(3)), boxes=boxes)
    assert boxes == [0]      # wholly nearer than near, by one unit in the last place
    at = np.array([[-0.4, -0.3, 0.5], [0.4, -0.3, 0.75], [0, 0.3, 1.0]], np.float32)      # a corner exactly at near: not in front of it
    boxes = []
    got = check(at, [[0, 1, 2]], EYE, K16, 12, 16, near=0.5, boxes=boxes)
    assert 0 < boxes[0] < 16 * 12 and (got[1] == 0).sum() > 10
    boxes = []
    check(at, [[0, 1, 2]], EYE, K16, 12, 16, near=np.nextafter(np.float32(0.5), np.float32(1)), boxes=boxes)
    assert boxes == [16 * 12]      # just behind near: the whole image


def test_equal_depths_go_to_the_smaller_index():
    v = np.array([[-1.5, -1.0, 2], [1.5, -1.0, 2], [0, 1.0, 2], [-1.0, 1.0, 2], [1.0, 1.0, 2], [0, -1.25, 2]], np.float32)
    a, b = [0, 1, 2], [3, 5, 4]      # two coplanar triangles that overlap, with opposite windings
    only_a, only_b = R.render(v, [a], EYE, K16, 12, 16)[1] == 0, R.render(v, [b], EYE, K16, 12, 16)[1] == 0
    overlap = only_a & only_b
    assert overlap.sum() > 10 and (only_a & ~only_b).sum() > 5 and (only_b & ~only_a).sum() > 5
    for faces, first, second in (([a, b], only_a, only_b), ([b, a], only_b, only_a)):
        depth, face = check(v, faces, EYE, K16, 12, 16)
        assert (face[first] == 0).all() and (face[second & ~first] == 1).all() and (depth[first | second] == 2).all()


# ---- many faces ---------------------------------------------------------------------------------------------------------------------------
def test_tilted_plane_equals_the_restatement_and_has_no_hole():
    vertices, faces = R.tilted_plane(0)
    depth, face = check(vertices, faces, EYE, R.PLANE_K, R.PLANE_H, R.PLANE_W)
    truth, inner = R.plane_truth()
    assert inner.sum() == 3012 and (face[inner] >= 0).all()      # shared edges leave no hole, whatever the windings and rotations
    assert (np.abs(depth[inner] - truth[inner]) / truth[inner]).max() <= 4 * 2.87e-6      # tests/test_mesh_depth_cpu.py measures the figure


CAMERAS = ["skew23", "skew140", "roll90", "pitch17"]      # scenes.CAMERAS: every entry of the rotation that hsr_camera_point reads is live


@pytest.mark.parametrize("camera", CAMERAS)
def test_tilted_plane_under_general_cameras(camera):
    """the plane placed with the inverse camera and rendered through the camera: m01, m10, m12, m21 of hsr_camera_point are 0 and m11 is 1
    under the identity and under a turn about y, here none is"""
    import scenes
    w2c = scenes.CAMERAS[camera]
    for seed in (0, 1):
        vertices, faces = R.tilted_plane(seed)
        depth, face = check(R.place(vertices, w2c), faces, w2c, R.PLANE_K, R.PLANE_H, R.PLANE_W)
        truth, inner = R.plane_truth()
        assert (face[inner] >= 0).all() and len(np.unique(face[face >= 0])) > 60
        if seed == 0:
            assert (np.abs(depth[inner] - truth[inner]) / truth[inner]).max() <= 4 * 2.87e-6      # as tests/test_mesh_depth_cpu.py holds the restatement


@pytest.mark.parametrize("camera", CAMERAS)
def test_random_faces_under_general_cameras(camera):
    """160 random faces on both sides of the split, two across the camera's plane, both windings (tests/test_mesh_depth_cpu.py holds the
    scene to that), placed with the inverse camera; and an odd image size through intrinsics with fx != fy"""
    import scenes
    w2c = scenes.CAMERAS[camera]
    vertices, faces = R.random_faces(3, R.PLANE_K, R.PLANE_H, R.PLANE_W)
    boxes = []
    depth, face = check(R.place(vertices, w2c), faces, w2c, R.PLANE_K, R.PLANE_H, R.PLANE_W, boxes=boxes)
    assert min(b for b in boxes if b) <= R.SMALL_BOX < max(boxes) and len(np.unique(face[face >= 0])) > 40
    k = np.array([[19.0, 0, 17.25], [0, 23.0, 20.5], [0, 0, 1]])
    vertices, faces = R.random_faces(4, k, 43, 37)
    depth, face = check(R.place(vertices, w2c), faces, w2c, k, 43, 37)
    assert len(np.unique(face[face >= 0])) > 30


@pytest.mark.parametrize("bad", [[0, 1, -1], [0, 1, 5], [0, 1, 3], [0, 1, 4], [0, 1, 1]], ids=["index-1", "indexV", "nan", "inf", "det0"])
def test_a_face_that_takes_no_part_beside_a_good_one(bad):
    v = np.concatenate([TRIANGLE, np.array([[0, 0, NAN], [INF, 0, 2]], np.float32)])
    alone = R.render(v, [[0, 1, 2]], EYE, K16, 12, 16)
    for faces, good in (([bad, [0, 1, 2]], 1), ([[0, 1, 2], bad], 0)):
        boxes = []
        depth, face = check(v, faces, EYE, K16, 12, 16, boxes=boxes)
        assert boxes[1 - good] == 0 and np.array_equal(bits(depth), bits(alone[0])) and np.array_equal(face, np.where(alone[1] == 0, good, -1))


def at_pixels(u, v, z, k):
    """the camera-space point that projects to (u, v) at depth z"""
    return [(u - k[0][2]) / k[0][0] * z, (v - k[1][2]) / k[1][1] * z, z]


# a box of exactly SMALL_BOX pixels and one of SMALL_BOX + 1, as (width, height), for the thresholds that were measured
THRESHOLD_BOXES = {64: ((8, 8), (5, 13)), 255: ((15, 17), (16, 16)), 1024: ((32, 32), (25, 41))}


def box_triangle(x0, y0, w, h):
    """pixel coordinates of a triangle whose box is x0 .. x0 + w - 1 by y0 .. y0 + h - 1: floor(min) - 1 .. ceil(max) + 1"""
    u0, u1, v0, v1 = x0 + 1.5, x0 + w - 2.5, y0 + 1.5, y0 + h - 2.5
    return [(u0, v0), (u1, v0), ((u0 + u1) / 2, v1)]


def test_both_paths_and_the_threshold_between_them():
    """257 faces of a pixel or two, one face whose box holds exactly SMALL_BOX pixels (the lane's last), one with SMALL_BOX + 1 (the
    sweep's first) and one that covers the whole image behind them all"""
    from hsr_utils import mesh_depth
    small = mesh_depth.SMALL_BOX
    assert small == R.SMALL_BOX and small in THRESHOLD_BOXES
    g = np.random.default_rng(7)
    centres = np.stack([g.uniform(1, 62, 257), g.uniform(1, 46, 257)], 1)
    vertices, faces = [], []
    for n, (u, v) in enumerate(centres):
        z = 1.0 + 0.01 * n
        vertices += [at_pixels(u + du, v + dv, z, K64) for du, dv in g.uniform(-1.2, 1.2, (3, 2))]
        faces.append([3 * n, 3 * n + 1, 3 * n + 2])
    (w0, h0), (w1, h1) = THRESHOLD_BOXES[small]
    special = [box_triangle(2, 3, w0, h0), box_triangle(36, 4, w1, h1) if w0 + w1 <= 58 else box_triangle(2, 3, w1, h1),
               [(-200.0, -100.0), (300.0, -100.0), (30.0, 400.0)]]
    for tri, z in zip(special, (3.0, 3.5, 5.0)):
        faces.append([len(vertices), len(vertices) + 1, len(vertices) + 2])
        vertices += [at_pixels(u, v, z, K64) for u, v in tri]
    vertices, faces = np.array(vertices, np.float32), np.array(faces, np.int32)
    boxes = []
    depth, face = check(vertices, faces, EYE, K64, 48, 64, boxes=boxes)
    assert boxes[257:] == [small, small + 1, 64 * 48] and 0 < max(boxes[:257]) <= 64 and len(faces) == 260
    assert (face >= 0).all() and {257, 258, 259} <= set(face.ravel().tolist())
    assert len(np.unique(face)) > 80      # a face of a pixel or two often holds no pixel centre


def test_three_hundred_faces_over_every_pixel():
    """300 whole-image faces at 300 distinct depths in a shuffled order: every pixel takes 300 candidates and keeps the nearest"""
    g = np.random.default_rng(11)
    depths = 2.0 + 0.01 * g.permutation(300)
    tri = [(-200.0, -100.0), (300.0, -100.0), (30.0, 400.0)]
    vertices = np.array([at_pixels(u, v, z, K64) for z in depths for u, v in tri], np.float32)
    faces = np.arange(900, dtype=np.int32).reshape(300, 3)
    boxes = []
    depth, face = check(vertices, faces, EYE, K64, 48, 64, boxes=boxes)
    assert boxes == [64 * 48] * 300 and (face == int(np.argmin(depths))).all() and (depth == 2).all()


def test_a_list_of_large_faces_longer_than_the_sweep_grid():
    """300 faces of about 22 pixels across, each with a box of more than SMALL_BOX pixels that lies inside the image, at depths of
    their own: every one is listed, the sweep's grid takes 128 listed faces at a time, so it goes round the list more than twice"""
    from hsr_utils import mesh_depth
    g = np.random.default_rng(13)
    vertices, faces = [], []
    for n in range(300):
        u, v, z = g.uniform(13, 50), g.uniform(13, 34), g.uniform(1.0, 4.0)
        corners = np.array([[-11, -10], [11, -10], [0, 11]]) + g.uniform(-1, 1, (3, 2))
        vertices += [at_pixels(u + du, v + dv, z + g.uniform(-0.2, 0.2), K64) for du, dv in corners]
        faces.append([3 * n, 3 * n + 1, 3 * n + 2] if n % 2 else [3 * n, 3 * n + 2, 3 * n + 1])
    boxes = []
    depth, face = check(np.array(vertices, np.float32), np.array(faces, np.int32), EYE, K64, 48, 64, boxes=boxes)
    assert len(boxes) == 300 > 128 and min(boxes) > mesh_depth.SMALL_BOX and max(boxes) < 64 * 48
    assert len(np.unique(face[face >= 0])) > 40      # faces of this size hide most of one another


def test_listed_boxes_of_more_than_one_round_of_the_sweep():
    """The sweep takes 16 x 256 = 4096 pixels of a box per round.  Six faces in an 80 x 64 image with boxes of 4200 to 4900 pixels, none
    as wide as the image and none with its corner at (0, 0), tilted so that they cut through one another: the second round of the
    walk through a box, where its column and row advance by a stride that is no multiple of the box's width, is compared bit for bit"""
    k = np.array([[32.0, 0, 39.5], [0, 32.0, 31.5], [0, 0, 1]])
    placed = [(4, 2, 70, 60), (3, 1, 75, 62), (9, 1, 66, 63), (1, 3, 77, 61), (6, 2, 73, 59), (2, 2, 71, 60)]
    g = np.random.default_rng(17)
    vertices, faces = [], []
    for n, (x0, y0, w, h) in enumerate(placed):
        tri = box_triangle(x0, y0, w, h)
        if n % 2:
            tri = [(u, 2 * y0 + h - 1 - v) for u, v in tri]      # every other one upside down, in the same box
        vertices += [at_pixels(u, v, g.uniform(1.5, 4.0), k) for u, v in tri]
        faces.append([3 * n, 3 * n + 1, 3 * n + 2] if n % 3 else [3 * n, 3 * n + 2, 3 * n + 1])
    boxes = []
    depth, face = check(np.array(vertices, np.float32), np.array(faces, np.int32), EYE, k, 64, 80, boxes=boxes)
    assert boxes == [w * h for _x, _y, w, h in placed] and min(boxes) > 16 * 256 and max(boxes) < 80 * 64
    assert len(np.unique(face[face >= 0])) >= 5 and (face >= 0).sum() > 3000 and (face[40:] >= 0).sum() > 500      # rows past the first round too


def test_no_faces_and_two_views_on_one_scratch():
    import scenes
    from hsr_utils import mesh_depth
    depth, face = check(TRIANGLE, np.zeros((0, 3), np.int32), EYE, K16, 12, 16)
    assert (depth == 0).all() and (face == -1).all()
    vertices, faces = R.tilted_plane(2)
    renderer = mesh_depth.MeshDepthRenderer(dev(vertices, torch.float32), dev(faces, torch.int32), R.PLANE_H, R.PLANE_W)
    away = np.eye(4)
    away[:3, 3] = [30.0, 0, 0]      # the plane is out of sight
    views = [EYE, scenes.tilted_w2c(), away, EYE] + [scenes.CAMERAS[n] for n in CAMERAS]
    got = [renderer.render(m, R.PLANE_K) for m in views]      # nothing is read between the calls
    for m, (d, f) in zip(views, got):
        want = R.render(vertices, faces, m, R.PLANE_K, R.PLANE_H, R.PLANE_W)
        assert np.array_equal(bits(d.cpu().numpy()), bits(want[0])) and np.array_equal(f.cpu().numpy(), want[1])
    assert (got[2][1] == -1).all() and (got[0][1] >= 0).sum() > 3000 and not torch.equal(got[0][1], got[1][1])
    assert sum(int((f >= 0).sum()) > 500 for _d, f in got[4:]) >= 3      # the general cameras see the plane too (skew140 looks away from it)
    with pytest.raises(ValueError, match="near must be finite and positive"):
        renderer.render(EYE, R.PLANE_K, near=0.0)
    with pytest.raises(RuntimeError, match=r"w2c must be \[4,4\]"):
        renderer.render(np.eye(3), R.PLANE_K)


# ---- Depth L1 -----------------------------------------------------------------------------------------------------------------------------
def test_depth_l1_of_a_mesh_against_itself_is_zero():
    import scenes
    from hsr_utils import mesh_depth
    vertices, faces = R.tilted_plane(3)
    mesh = (dev(vertices, torch.float32), dev(faces, torch.int32))
    got = mesh_depth.mesh_depth_l1(mesh, (vertices, faces), np.stack([EYE, scenes.tilted_w2c()]), R.PLANE_K, R.PLANE_H, R.PLANE_W)
    assert got["depth_l1"] == 0.0 and got["depth_l1_covered"] == 0.0 and got["gt_cover"] == got["rec_cover"] == got["both_cover"] > 0.5
    assert got["per_view_l1"].dtype == np.float64 and got["per_view_l1"].tolist() == [0.0, 0.0]


def test_depth_l1_of_a_room_with_its_far_wall_moved():
    """from the middle of a 4 x 3 x 6 m room, looking along z with a field of view that the far wall fills: moving that wall by 0.01 m
    along the axis moves every depth by 0.01; the bound is the float32 spacing at 3 m (2.4e-7) times a handful of roundings"""
    from hsr_utils import mesh_depth
    k = np.array([[60.0, 0, 31.5], [0, 60.0, 23.5], [0, 0, 1]])
    gt, rec = R.box_room(), R.box_room(far=3.01)
    assert len(gt[1]) == 12
    gt_dev, rec_dev = tuple(dev(a, t) for a, t in zip(gt, (torch.float32, torch.int32))), tuple(dev(a, t) for a, t in zip(rec, (torch.float32, torch.int32)))
    got = mesh_depth.mesh_depth_l1(rec_dev, gt_dev, EYE[None], k, 48, 64)
    depth, face = mesh_depth.render_mesh_depth(*gt_dev, EYE, k, 48, 64)
    assert set(face.unique().tolist()) == {2, 3} and float((depth - 3.0).abs().max()) <= 1e-6      # the view sees only that wall
    print(got)
    assert abs(got["depth_l1_covered"] - 0.01) <= 1e-5 and abs(got["depth_l1"] - 0.01) <= 1e-5
    assert got["gt_cover"] == got["rec_cover"] == got["both_cover"] == 1.0 and abs(got["per_view_l1"][0] - 0.01) <= 1e-5
    # from outside, looking away from the room, nothing is hit: the covered mean has no pixels
    out = np.eye(4)
    out[2, 3] = -10.0
    none = mesh_depth.mesh_depth_l1(rec_dev, gt_dev, out[None], k, 48, 64)
    assert none["depth_l1"] == 0.0 and np.isnan(none["depth_l1_covered"]) and none["both_cover"] == 0.0


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
NEW_KEYS = {"depth_l1", "depth_l1_covered", "depth_gt_cover", "depth_rec_cover", "depth_views"}


def test_a_run_against_its_own_mesh_from_virtual_views(session, tmp_path):  # noqa: F811
    own = session.export_mesh(str(tmp_path / "own.ply"), voxel_size=VOXEL, every=EVERY)
    plain = session.evaluate_mesh(own[0], **SCORE)
    first = session.evaluate_mesh(own[0], depth_views=4, depth_size=(48, 64), **SCORE)
    again = session.evaluate_mesh(own[0], depth_views=4, depth_size=(48, 64), **SCORE)
    assert not NEW_KEYS & set(plain) and set(first) == set(again) == set(plain) | NEW_KEYS
    print({n: first[n] for n in sorted(NEW_KEYS)})
    for name in first:      # the same numbers from two calls, and the old numbers unchanged by the new ones
        same = torch.equal(first[name], again[name]) if isinstance(first[name], torch.Tensor) else first[name] == again[name]
        assert same, name
        if name in plain:
            assert torch.equal(first[name], plain[name]) if isinstance(first[name], torch.Tensor) else first[name] == plain[name], name
    assert first["depth_views"] == 4 and 0 <= first["depth_l1_covered"] < VOXEL and 0 <= first["depth_l1"]
    assert 0 < first["depth_gt_cover"] <= 1 and 0 < first["depth_rec_cover"] <= 1
    other = session.evaluate_mesh(own[0], depth_views=4, depth_seed=5, **SCORE)      # the run's own size, other views
    assert set(other) == set(first) and 0 <= other["depth_l1_covered"] < VOXEL and other["depth_gt_cover"] != first["depth_gt_cover"]


def test_the_tool_reports_depth_l1_in_a_fresh_process(session, sequence, tmp_path):  # noqa: F811
    from hsr_utils import map_io, mesh_eval
    s = session
    cam, intrinsics, frames = sequence
    out = map_io.finalize_params(s.params, s.variables, intrinsics, torch.eye(4), TS.W, TS.H, [f["gt_w2c"] for f in frames], s.keyframe_time_indices)
    saved = map_io.save_params(out, str(tmp_path / "run"))
    own = s.export_mesh(str(tmp_path / "own.ply"), voxel_size=VOXEL, every=EVERY)
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "eval_mesh.py")
    common = [sys.executable, tool, saved, own[0], "--voxel-size", str(VOXEL), "--every", str(EVERY), "--threshold", str(2 * VOXEL), "--samples", "20000",
              "--semantic"]
    done = subprocess.run(common + ["--depth-views", "4", "--depth-seed", "3", "--depth-size", "48", "64"], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    score = json.loads(done.stdout.strip().splitlines()[-1])
    assert NEW_KEYS <= set(score) and score["depth_views"] == 4
    params = map_io.load_params(saved, device="cuda")
    again = mesh_eval.evaluate_mesh_run(params, own[0], semantic=True, depth_views=4, depth_seed=3, depth_size=(48, 64), **SCORE)
    for name in sorted(NEW_KEYS):
        assert score[name] == again[name], name
    assert float(again["completion"]) == score["completion"] and 0 <= score["depth_l1_covered"] < VOXEL
    without = mesh_eval.evaluate_mesh_run(params, own[0], semantic=True, **SCORE)
    assert not NEW_KEYS & set(without) and set(without) | NEW_KEYS == set(again)
