"""GPU suite for the pictures of a mesh (include/shade/hsr_mesh_shade.h, hsr_utils.mesh_view): the vertex normals and every picture
against the numpy restatement of tests/mesh_view_ref.py, BIT FOR BIT, at the smallest sizes at which the kernels can go wrong: faces
that take no part, two thousand faces meeting at one vertex, every kind flat and smooth, lit and unlit, faces across the camera's plane,
a view that sees nothing, face images with indices that are not the mesh's, labels and scalars at their edges, the odd tail of the
four-pixel layout and an out that is off four bytes; the renderer against the raw calls, the files against the tensors, the errors
against brute force, a fused sphere end to end; and hsr_mesh_depth still against its own restatement after the move of its face
functions into csrc/hsr_mesh_face.h."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mesh_depth_ref as D
import mesh_eval_ref
import mesh_view_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN, INF = float("nan"), float("inf")
EYE = np.eye(4)
K, H, W = D.PLANE_K, D.PLANE_H, D.PLANE_W      # 64 x 48


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    return t if dtype is None else t.to(dtype)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the raw calls ------------------------------------------------------------------------------------------------------------------------
def device_normals(vertices, faces):
    """hsr_mesh_normals into a fresh scratch filled with 0xFF: float32 [V,3]"""
    from diff_gaussian_rasterization import _abi
    v, f = dev(vertices, torch.float32), dev(np.asarray(faces).reshape(-1, 3), torch.int32)
    size = _abi.lib.hsr_mesh_normals_scratch_bytes(len(v))
    scratch = torch.full((size,), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.full((len(v), 3), NAN, dtype=torch.float32, device=DEV)
    _abi.call(_abi.lib.hsr_mesh_normals, "hsr_mesh_normals", v.device, len(v), len(f), v.data_ptr(), f.data_ptr() if len(f) else None,
              scratch.data_ptr(), size, out.data_ptr())
    return out.cpu().numpy()


def device_shade(vertices, faces, w2c, k, h, w, face_image, jobs, offset=0):
    """hsr_mesh_shade for R.job dictionaries: a list of uint8 [h,w,3]; offset: every out starts that many bytes into its buffer"""
    from diff_gaussian_rasterization import _abi
    v, f = dev(vertices, torch.float32), dev(np.asarray(faces).reshape(-1, 3), torch.int32)
    image = dev(face_image, torch.int32)
    array = (_abi.hsr_shade_job * len(jobs))()
    keep, outs = [], []
    for job, j in zip(array, jobs):
        job.kind, job.lit, job.ambient, job.lo, job.hi = j["kind"], int(j["lit"]), j["ambient"], j["lo"], j["hi"]
        job.albedo[:] = list(j["albedo"])
        job.background[:] = list(j["background"]) + [0]
        for field, dtype in (("normals", torch.float32), ("attr", {R.COLOUR: torch.uint8, R.LABELS: torch.int32}.get(j["kind"], torch.float32)),
                             ("table", torch.uint8)):
            if j[field] is not None:
                keep.append(dev(j[field], dtype))
                setattr(job, field, keep[-1].data_ptr())
        job.n = 0 if j["table"] is None else len(j["table"])
        outs.append(torch.full((h * w * 3 + 8,), 0x5A, dtype=torch.uint8, device=DEV))
        job.out = outs[-1].data_ptr() + offset
    m = np.ascontiguousarray(w2c, np.float32)
    fx, fy, cx, cy = (float(x) for x in D.pinhole(k))
    _abi.call(_abi.lib.hsr_mesh_shade, "hsr_mesh_shade", v.device, len(v), len(f), v.data_ptr(), f.data_ptr() if len(f) else None, h, w, fx, fy,
              cx, cy, m.ctypes.data_as(_abi.fp), image.data_ptr(), len(jobs), array)
    got = [o.cpu().numpy() for o in outs]
    for o in got:      # nothing before the picture, nothing after it
        assert (o[:offset] == 0x5A).all() and (o[offset + h * w * 3:] == 0x5A).all()
    return [o[offset:offset + h * w * 3].reshape(h, w, 3) for o in got]


def device_depth(vertices, faces, w2c, k, h, w, near=0.01):
    from hsr_utils import mesh_depth
    depth, face = mesh_depth.render_mesh_depth(dev(vertices, torch.float32), dev(np.asarray(faces).reshape(-1, 3), torch.int32), w2c, k, h, w, near)
    return depth.cpu().numpy(), face.cpu().numpy()


# ---- vertex normals -----------------------------------------------------------------------------------------------------------------------
def normal_scenes():
    faces_v, faces_f = D.random_faces(3, K, H, W, n=160)
    return {"sphere": R.sphere(2), "box_room": D.box_room(), "random_faces": R.take_no_part(faces_v, faces_f), "fan": R.fan(2000)}


@pytest.mark.parametrize("scene", ["sphere", "box_room", "random_faces", "fan"])
def test_normals_equal_the_restatement_on_every_run(scene):
    vertices, faces = normal_scenes()[scene]
    want = R.normals(vertices, faces)
    first, second = device_normals(vertices, faces), device_normals(vertices, faces)
    assert np.array_equal(bits(first), bits(want)), np.abs(first - want).max()
    assert np.array_equal(bits(first), bits(second))
    length = np.linalg.norm(want.astype(np.float64), axis=1)
    assert ((np.abs(length - 1) < 1e-6) | (length == 0)).all() and (length > 0).sum() >= 8
    if scene == "random_faces":      # the seven faces that take no part leave their own vertices at zero
        untouched = [3 * i + j for i in (5, 17, 40, 60, 61, 90, 91) for j in range(3)]
        assert (want[untouched] == 0).all() and (length > 0).sum() == 3 * 153
    if scene == "fan":
        assert length[0] > 0 and abs(want[0][2]) > 0.9      # two thousand faces met at the hub


def test_normals_of_no_faces_are_zero():
    got = device_normals(R.sphere(1)[0], np.zeros((0, 3), np.int32))
    assert got.shape == (18, 3) and np.array_equal(bits(got), np.zeros((18, 3), np.uint32))
    from hsr_utils import mesh_view
    vertices, faces = R.sphere(2)
    assert np.array_equal(bits(mesh_view.vertex_normals(dev(vertices), dev(faces)).cpu().numpy()), bits(R.normals(vertices, faces)))


# ---- the pictures -------------------------------------------------------------------------------------------------------------------------
def inside_room():
    """the box room seen from inside, off its middle and turned: faces cross z = near, half the mesh is behind the camera"""
    import scenes
    w2c = np.array(scenes.CAMERAS["skew23"], np.float64)
    w2c[:3, 3] = [0.3, -0.2, 0.4]
    return D.box_room() + (w2c,)


def picture_scenes():
    plane_v, plane_f = D.tilted_plane(0)
    faces_v, faces_f = D.random_faces(3, K, H, W, n=160)
    room_v, room_f, room_w2c = inside_room()
    return {"tilted_plane": (plane_v, plane_f, EYE), "random_faces": (faces_v, faces_f, EYE), "box_room": (room_v, room_f, room_w2c),
            "nothing": (plane_v * np.float32([1, 1, -1]), plane_f, EYE)}


def all_jobs(vertices, faces, n_labels=7):
    """every kind, flat and smooth, lit and unlit: twenty jobs, with labels at n, -1 and n - 1 and scalars at NaN, +inf, lo and hi"""
    V = len(vertices)
    rgb, labels, scalar = R.attributes(V, 1, n_labels)
    labels[::5], labels[1::7], labels[2::9] = n_labels, -1, n_labels - 1
    scalar[::6], scalar[1::8], scalar[2::10], scalar[3::11] = NAN, INF, -0.25, 1.25      # lo and hi themselves
    smooth = R.normals(vertices, faces)
    table, jet = R.table(n_labels, 2), R.table(256, 3)
    jobs = []
    for normals in (None, smooth):
        for lit in (True, False):
            common = dict(normals=normals, lit=lit, ambient=0.25 if lit else 0.4, background=(255, 255, 255) if lit else (10, 20, 30))
            jobs += [R.job("shaded", albedo=(0.8, 0.7, 0.55), **common), R.job("colour", attr=rgb, **common), R.job("normals", **common),
                     R.job("labels", attr=labels, table=table, **common), R.job("scalar", attr=scalar, table=jet, lo=-0.25, hi=1.25, **common)]
    return jobs


@pytest.mark.parametrize("scene", ["tilted_plane", "random_faces", "box_room", "nothing"])
def test_every_kind_equals_the_restatement(scene):
    vertices, faces, w2c = picture_scenes()[scene]
    depth, face = device_depth(vertices, faces, w2c, K, H, W)
    want_depth, want_face = D.render(vertices, faces, w2c, K, H, W)
    assert np.array_equal(bits(depth), bits(want_depth)) and np.array_equal(face, want_face)      # hsr_mesh_depth after the move of its face functions
    hit = face >= 0
    if scene == "nothing":
        assert not hit.any()
    elif scene == "box_room":
        boxes = []
        D.render(vertices, faces, w2c, K, H, W, boxes=boxes)
        assert hit.all() and boxes.count(H * W) >= 2 and boxes.count(0) >= 2      # faces across z = near, faces behind the camera
    else:
        assert 0.5 < hit.mean() < 1 and len(np.unique(face[hit])) > 40
    jobs = all_jobs(vertices, faces)
    terms = R.pixel_terms(vertices, faces, w2c, K, H, W, face)
    assert np.array_equal(terms["hit"].reshape(H, W), hit)      # no pixel of hsr_mesh_depth's own face image fails the shade's clauses
    want = R.shade(vertices, faces, w2c, K, H, W, face, jobs, terms=terms)
    got = []
    for start in (0, 8, 16):      # twenty jobs in calls of 8, 8 and 4
        got += device_shade(vertices, faces, w2c, K, H, W, face, jobs[start:start + 8])
    for i, (g, w_, j) in enumerate(zip(got, want, jobs)):
        assert np.array_equal(g, w_), (scene, i, j["kind"], j["lit"], j["normals"] is not None, int((g != w_).any(-1).sum()))
        assert (g[~hit] == np.array(j["background"], np.uint8)).all()
    if scene in ("tilted_plane", "random_faces"):      # the pictures are pictures: the kinds differ, and lit differs from unlit
        assert len({g.tobytes() for g in got[:5]}) == 5
        assert not np.array_equal(got[1], got[6]) and not np.array_equal(got[3], got[8]) and not np.array_equal(got[4], got[9])
        assert (got[3][hit] == 0).all(-1).any()      # a label outside the table is black
    if scene == "tilted_plane":      # its faces share vertices and are wound at random: smooth differs from flat (random_faces shares none)
        assert not np.array_equal(got[0], got[10]) and not np.array_equal(got[2], got[12])


def test_eight_jobs_in_one_call_equal_eight_calls():
    vertices, faces, w2c = picture_scenes()["random_faces"]
    face = device_depth(vertices, faces, w2c, K, H, W)[1]
    jobs = all_jobs(vertices, faces)[7:15]      # both normals, lit and unlit, every kind among them
    together = device_shade(vertices, faces, w2c, K, H, W, face, jobs)
    for j, t in zip(jobs, together):
        assert np.array_equal(device_shade(vertices, faces, w2c, K, H, W, face, [j])[0], t)


def test_foreign_face_indices_give_background_at_exactly_those_pixels():
    vertices, faces = R.take_no_part(*D.random_faces(3, K, H, W, n=160))
    face = device_depth(vertices, faces, EYE, K, H, W)[1]
    hit = np.flatnonzero(face.reshape(-1) >= 0)
    assert len(hit) > 1000 and not np.isin(face, [5, 17, 40, 91]).any()      # faces that take no part are in no pixel
    foreign = face.reshape(-1).copy()
    chosen = hit[:: len(hit) // 40][:36]
    for n, value in enumerate((-1, len(faces), 2 ** 31 - 1, -2 ** 31, 5, 17, 40, 91, len(faces) + 7)):      # 5, 17, 40: an index outside the vertices; 91: a cross that is not finite
        foreign[chosen[n::9]] = value
    jobs = all_jobs(vertices, faces)[:8]
    want = R.shade(vertices, faces, EYE, K, H, W, foreign, jobs)
    got = device_shade(vertices, faces, EYE, K, H, W, foreign, jobs)
    clean = device_shade(vertices, faces, EYE, K, H, W, face, jobs)
    rest = np.setdiff1d(np.arange(H * W), chosen)
    for g, w_, c, j in zip(got, want, clean, jobs):
        assert np.array_equal(g, w_)
        assert (g.reshape(-1, 3)[chosen] == np.array(j["background"], np.uint8)).all()
        assert np.array_equal(g.reshape(-1, 3)[rest], c.reshape(-1, 3)[rest])
    other_v, other_f = D.tilted_plane(0)      # a face image from another mesh altogether: 128 faces against this mesh's 160, and the other way round
    other_face = device_depth(other_v, other_f, EYE, K, H, W)[1]
    assert np.array_equal(device_shade(vertices, faces, EYE, K, H, W, other_face, jobs[:3])[0], R.shade(vertices, faces, EYE, K, H, W, other_face, jobs[:3])[0])
    plane_jobs = all_jobs(other_v, other_f)[:5]
    for g, w_ in zip(device_shade(other_v, other_f, EYE, K, H, W, face, plane_jobs), R.shade(other_v, other_f, EYE, K, H, W, face, plane_jobs)):
        assert np.array_equal(g, w_) and (g.reshape(-1, 3)[face.reshape(-1) >= 128] == 255).all()


def test_wild_vertex_indices_and_attribute_edges():
    """a mesh whose faces point outside the vertices, next to good ones; labels at n, -1, n - 1 and scalars at NaN, +inf, lo, hi on a
    single triangle, where each corner's value can be told"""
    v = np.array([[-1.5, -1.0, 2], [1.5, -1.0, 2], [0, 1.0, 2], [0, 0, 1]], np.float32)
    k = np.array([[8.0, 0, 7.5], [0, 8.0, 5.5], [0, 0, 1]])
    faces = np.array([[0, 1, 2], [0, 1, 4], [-1, 1, 2], [2 ** 31 - 1, 0, 1]], np.int32)
    table, jet = R.table(3, 4), R.table(256, 5)
    for labels, scalar in (([3, -1, 2, 0], [NAN, 0, 0, 0]), ([2, 3, -1, 0], [INF, 0.5, 0.5, 0]), ([0, 1, 2, 0], [0.25, 0.75, 0.25, 0]),
                           ([-2 ** 31, 2 ** 31 - 1, 1, 0], [-INF, 0.25, 0.75, 0])):
        jobs = [R.job("labels", attr=np.array(labels, np.int32), table=table, lit=lit) for lit in (False, True)]
        jobs += [R.job("scalar", attr=np.array(scalar, np.float32), table=jet, lo=0.25, hi=0.75, lit=lit) for lit in (False, True)]
        for image in (np.zeros((12, 16), np.int32), np.arange(12 * 16, dtype=np.int32).reshape(12, 16) % 5 - 1):      # every face, and -1 and 4
            want = R.shade(v, faces, EYE, k, 12, 16, image, jobs)
            got = device_shade(v, faces, EYE, k, 12, 16, image, jobs)
            for g, w_ in zip(got, want):
                assert np.array_equal(g, w_)
            assert (got[0][image != 0] == 255).all()      # faces 1..3 have wild indices: background
    face = D.render(v, faces, EYE, k, 12, 16)[1]
    lab = device_shade(v, faces, EYE, k, 12, 16, face, [R.job("labels", attr=np.array([3, -1, 2, 0], np.int32), table=table, lit=False)])[0]
    assert {tuple(c) for c in lab[face == 0].tolist()} == {(0, 0, 0), tuple(table[2].tolist())}      # n and -1 are black, n - 1 is the last row
    sca = device_shade(v, faces, EYE, k, 12, 16, face, [R.job("scalar", attr=np.array([0.25, 0.75, 0.25, 0], np.float32), table=jet, lo=0.25, hi=0.75, lit=False)])[0]
    seen = {tuple(c) for c in sca[face == 0].tolist()}
    assert len(seen) > 20 and seen <= {tuple(r) for r in jet.tolist()}      # between lo and hi: rows of the table, many of them


@pytest.mark.parametrize("h,w", [(7, 1), (5, 3), (3, 64), (5, 67)])
def test_image_widths_and_the_odd_tail(h, w):
    k = np.array([[20.0, 0, (w - 1) / 2], [0, 20.0, (h - 1) / 2], [0, 0, 1]])
    vertices, faces = D.random_faces(5, k, h, w, n=40)
    face = D.render(vertices, faces, EYE, k, h, w)[1]
    assert (face >= 0).any() and h * w % 4 == {(7, 1): 3, (5, 3): 3, (3, 64): 0, (5, 67): 3}[(h, w)]
    jobs = all_jobs(vertices, faces)[5:13]
    want = R.shade(vertices, faces, EYE, k, h, w, face, jobs)
    for offset in (0, 4, 1, 2, 3):      # an out on four bytes takes the four-pixel kernel, an out off them the one-pixel kernel
        for g, w_ in zip(device_shade(vertices, faces, EYE, k, h, w, face, jobs, offset=offset), want):
            assert np.array_equal(g, w_), (h, w, offset)


def test_one_misaligned_out_among_aligned_ones():
    from diff_gaussian_rasterization import _abi
    vertices, faces, w2c = picture_scenes()["tilted_plane"]
    face = device_depth(vertices, faces, w2c, K, H, W)[1]
    jobs = all_jobs(vertices, faces)[:3]
    want = R.shade(vertices, faces, w2c, K, H, W, face, jobs)
    v, f, image = dev(vertices, torch.float32), dev(faces, torch.int32), dev(face, torch.int32)
    array = (_abi.hsr_shade_job * 3)()
    buffers = [torch.zeros(H * W * 3 + 8, dtype=torch.uint8, device=DEV) for _ in jobs]
    for n, (job, j) in enumerate(zip(array, jobs)):
        job.kind, job.lit, job.ambient = j["kind"], 1, j["ambient"]
        job.albedo[:] = list(j["albedo"])
        job.background[:] = [255, 255, 255, 0]
        job.out = buffers[n].data_ptr() + (3 if n == 1 else 0)      # the second picture alone is off four bytes
    rgb = dev(jobs[1]["attr"], torch.uint8)
    array[1].attr = rgb.data_ptr()
    m = np.ascontiguousarray(w2c, np.float32)
    _abi.call(_abi.lib.hsr_mesh_shade, "hsr_mesh_shade", v.device, len(v), len(f), v.data_ptr(), f.data_ptr(), H, W, *(float(x) for x in D.pinhole(K)),
              m.ctypes.data_as(_abi.fp), image.data_ptr(), 3, array)
    for n, w_ in enumerate(want):
        start = 3 if n == 1 else 0
        assert np.array_equal(buffers[n].cpu().numpy()[start:start + H * W * 3].reshape(H, W, 3), w_)


# ---- the module ---------------------------------------------------------------------------------------------------------------------------
def test_renderer_equals_the_raw_calls_and_files_hold_the_tensors(tmp_path):
    from PIL import Image
    from hsr_utils import export, mesh_view
    vertices, faces, w2c = picture_scenes()["random_faces"]
    rgb, labels, scalar = R.attributes(len(vertices), 1)
    renderer = mesh_view.MeshRenderer(dev(vertices), dev(faces), H, W, rgb=dev(rgb), labels=dev(labels))
    assert np.array_equal(bits(renderer.normals.cpu().numpy()), bits(R.normals(vertices, faces)))
    names = ("shaded", "colour", "normals", "labels", "scalar")
    got = renderer.render(w2c, K, names, scalar=dev(scalar), scalar_range=(0.0, 1.0))
    assert sorted(got) == sorted(names + ("depth", "face"))
    depth, face = device_depth(vertices, faces, w2c, K, H, W)
    assert np.array_equal(bits(got["depth"].cpu().numpy()), bits(depth)) and np.array_equal(got["face"].cpu().numpy(), face)
    smooth = R.normals(vertices, faces)
    jobs = [R.job("shaded", normals=smooth), R.job("colour", normals=smooth, attr=rgb), R.job("normals", normals=smooth),
            R.job("labels", normals=smooth, attr=labels, table=export.label_colormap(256, "cpu").numpy()),
            R.job("scalar", normals=smooth, attr=scalar, table=export.jet_colormap("cpu").numpy(), lo=0.0, hi=1.0)]
    for name, raw in zip(names, device_shade(vertices, faces, w2c, K, H, W, face, jobs)):
        assert got[name].dtype == torch.uint8 and got[name].shape == (H, W, 3) and got[name].is_cuda
        assert np.array_equal(got[name].cpu().numpy(), raw), name
    flat = mesh_view.MeshRenderer(dev(vertices), dev(faces), H, W, normals="flat").render(w2c, K, "shaded", lit=False, background=(1, 2, 3))
    assert np.array_equal(flat["shaded"].cpu().numpy(), device_shade(vertices, faces, w2c, K, H, W, face, [R.job("shaded", background=(1, 2, 3))])[0])
    with pytest.raises(RuntimeError, match="needs the mesh's rgb"):
        mesh_view.MeshRenderer(dev(vertices), dev(faces), H, W).render(w2c, K, ("colour",))
    with pytest.raises(ValueError, match="pictures must be"):
        renderer.render(w2c, K, ("shaded", "wireframe"))
    # the views of a list, as tensors and as files
    views = np.stack([np.asarray(w2c, np.float32), np.asarray(w2c, np.float32)])
    views[1][0, 3] += 0.25
    mesh = (dev(vertices), dev(faces), dev(rgb), dev(labels))
    gt_v, gt_f = D.tilted_plane(0)
    tensors = mesh_view.render_mesh_views(mesh, views, K, H, W, pictures=("shaded", "colour"), gt=(dev(gt_v), dev(gt_f)))
    assert len(tensors) == 2 and np.array_equal(tensors[0]["shaded"].cpu().numpy(), got["shaded"].cpu().numpy())
    assert not np.array_equal(tensors[1]["shaded"].cpu().numpy(), got["shaded"].cpu().numpy())
    paths = mesh_view.render_mesh_views(mesh, views, K, H, W, out_dir=str(tmp_path), pictures=("shaded", "colour"), gt=(dev(gt_v), dev(gt_f)))
    want_names = ["%s_%04d.png" % (p, i) for i in range(2) for p in ("shaded", "colour", "gt_shaded")]
    assert [os.path.basename(p) for p in paths] == want_names and sorted(os.listdir(tmp_path)) == sorted(want_names)
    for i in range(2):
        for p in ("shaded", "colour", "gt_shaded"):
            assert np.array_equal(np.asarray(Image.open(os.path.join(tmp_path, "%s_%04d.png" % (p, i)))), tensors[i][p].cpu().numpy())
    # the heat map: "scalar" without a scalar is the mesh's distance to samples of the ground truth
    heat = mesh_view.render_mesh_views(mesh, views[:1], K, H, W, pictures=("scalar",), gt=(dev(gt_v), dev(gt_f)), error_samples=2000)
    assert heat[0]["scalar"].shape == (H, W, 3) and len(torch.unique(heat[0]["scalar"].reshape(-1, 3), dim=0)) > 10


def test_vertex_errors_equal_brute_force():
    """500 vertices against 800 points: the squared distances are mesh_eval's, exact; the root is torch's, whose rounding this project
    does not pin, so it is compared within 2 ulp"""
    from hsr_utils import mesh_view
    rng = np.random.default_rng(7)
    vertices, points = rng.uniform(-1, 1, (500, 3)).astype(np.float32), rng.uniform(-1, 1, (800, 3)).astype(np.float32)
    vertices[17] = [NAN, 0, 0]
    want = np.sqrt(mesh_eval_ref.brute_nn(vertices, points)[0])
    for cell in (None, 0.3):
        got = mesh_view.vertex_errors(dev(vertices), dev(points), cell=cell).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (500,) and got[17] == INF
        assert np.abs(got[want < INF] - want[want < INF]).max() <= 2 * np.spacing(want[want < INF].max())


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
SPHERE_R = 0.5
MEAN_ANGLE_64 = 2.047682e-1      # radians (11.7 degrees): measured once from the float64 restatement on the extracted mesh (see the test)


def sphere_depth(w2c, k, h, w):
    """float32 [h,w]: the depth along the camera's axis at which the ray of every pixel centre meets the sphere of radius SPHERE_R round
    the origin; 0 where it misses"""
    m = np.asarray(w2c, np.float64)
    c = m[:3, 3]      # the sphere's centre in camera space
    ys, xs = np.mgrid[0:h, 0:w]
    ray = np.stack([(xs - k[0][2]) / k[0][0], (ys - k[1][2]) / k[1][1], np.ones((h, w))], -1)
    a, b, cc = (ray * ray).sum(-1), -2 * (ray @ c), c @ c - SPHERE_R ** 2
    disc = b * b - 4 * a * cc
    t = (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a)
    return np.where(disc > 0, t, 0).astype(np.float32)


def test_fused_sphere_end_to_end():
    """A sphere of radius 0.5 fused into a 32^3 TsdfVolume from four views on a circle round it (orbit_views), extracted, and rendered
    "normals" and "shaded" from the first of them with smooth normals.  Every hit pixel's shading normal faces the camera, and the mean
    angle between it and the analytic normal of the sphere at the hit point stays within 1.01 times MEAN_ANGLE_64: that figure was
    measured once by this test's own float64 restatement (normals64 and shading_normals64 on the extracted mesh) and is printed on every
    run next to the device's (2.047670e-1 when it was measured).  It is the mesh's figure, not the arithmetic's: a 32^3 volume fused from
    four projective views of 128 x 96 pixels gives a faceted sphere.  The 1 % is for the float32 normals and weights, which move a
    pixel's normal by about 1e-6, and for nothing else — the mesh is the device's own and the same on every run."""
    from hsr_utils import mesh, mesh_view
    h, w = 96, 128
    k = np.array([[160.0, 0, 63.5], [0, 160.0, 47.5], [0, 0, 1]])
    views = mesh_view.orbit_views([-SPHERE_R] * 3, [SPHERE_R] * 3, 4, elevation_deg=20.0, distance=2.0)
    step = 1.4 / 31
    vol = mesh.TsdfVolume((-0.7, -0.7, -0.7), (32, 32, 32), step, color=False)
    for m in views:
        vol.integrate(dev(sphere_depth(m, k, h, w)), m, k)
    vertices, faces, _rgb, _labels = vol.extract()
    assert len(faces) > 1000
    got = mesh_view.MeshRenderer(vertices, faces, h, w).render(views[0], k, ("normals", "shaded"))
    v_np, f_np, face = vertices.cpu().numpy(), faces.cpu().numpy(), got["face"].cpu().numpy()
    hit = face.reshape(-1) >= 0
    assert hit.sum() > 2000
    smooth = R.normals(v_np, f_np)
    terms = R.pixel_terms(v_np, f_np, views[0], k, h, w, face)
    want = R.shade(v_np, f_np, views[0], k, h, w, face, [R.job("normals", normals=smooth), R.job("shaded", normals=smooth)], terms=terms)
    assert np.array_equal(got["normals"].cpu().numpy(), want[0]) and np.array_equal(got["shaded"].cpu().numpy(), want[1])
    n = R.shading_normal(terms, views[0], smooth)[hit].astype(np.float64)      # what the device's bytes were made from, bit for bit
    view = terms["v"][hit].astype(np.float64)
    assert ((n * view).sum(1) > 0).all()      # every hit pixel's normal faces the camera
    m = views[0].astype(np.float64)

    def mean_angle(normal, point):
        world = (point - m[:3, 3]) @ m[:3, :3]      # the hit point back in the world: the sphere is round its origin
        analytic = (world / np.linalg.norm(world, axis=1, keepdims=True)) @ m[:3, :3].T
        return float(np.arccos(np.clip((normal * analytic).sum(1), -1, 1)).mean())

    n64, p64 = R.shading_normals64(v_np, f_np, views[0], k, h, w, face, R.normals64(v_np, f_np))
    angle, angle64 = mean_angle(n, terms["p"][hit].astype(np.float64)), mean_angle(n64[hit], p64[hit])
    print("mean angle to the sphere's normal: device rule %.6e rad, float64 restatement %.6e rad over %d pixels" % (angle, angle64, hit.sum()))
    assert abs(angle64 - MEAN_ANGLE_64) <= 1e-3 * MEAN_ANGLE_64      # the figure stated above is this mesh's
    assert angle <= 1.01 * MEAN_ANGLE_64
    shaded = got["shaded"].cpu().numpy().reshape(-1, 3)
    assert (shaded[~hit] == 255).all() and shaded[hit].max() > 180 and shaded[hit].min() >= 50      # ambient 0.25 of albedo 0.8 is 51


# ---- hsr_mesh_depth after the move of its face functions ----------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["random_faces", "box_room"])
def test_mesh_depth_still_equals_its_restatement(scene):
    vertices, faces, w2c = picture_scenes()[scene]
    for near in (0.01, 0.8):
        depth, face = device_depth(vertices, faces, w2c, K, H, W, near)
        want = D.render(vertices, faces, w2c, K, H, W, near)
        assert np.array_equal(bits(depth), bits(want[0])) and np.array_equal(face, want[1])
    import scenes
    for camera in ("skew140", "roll90"):
        m = scenes.CAMERAS[camera]
        world = D.place(vertices, m) if scene == "random_faces" else vertices
        depth, face = device_depth(world, faces, m, K, H, W)
        want = D.render(world, faces, m, K, H, W)
        assert np.array_equal(bits(depth), bits(want[0])) and np.array_equal(face, want[1])
