"""CPU suite for the pictures of a mesh (include/shade/hsr_mesh_shade.h, hsr_utils.mesh_view): the header through the helpers of
tests/test_abi.py (its prototypes, that the library exports them and that _abi.SHADE_HEADERS binds them with the header's types, the job
struct against its typedef); every refusal of both entry points with dummy pointers; the scratch size; the lazy names; orbit_views
against the construction its docstring states; the numpy restatement (tests/mesh_view_ref.py) against analysis — the normals of a
sphere, the weights of a plane, a linear colour; the tool's options.  Nothing here launches: there is no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import mesh_depth_ref as D
import mesh_view_ref as R
import test_abi

HEADER = "shade/hsr_mesh_shade.h"
NAMES = ["hsr_mesh_normals_scratch_bytes", "hsr_mesh_normals", "hsr_mesh_shade"]
FP, VP, IP = ("pointer", "float"), ("pointer", "void"), ("pointer", "int")
NAN, INF = float("nan"), float("inf")


def tables():
    from diff_gaussian_rasterization import _abi
    return (_abi.HEADERS, _abi.EVAL_HEADERS, _abi.RECON_HEADERS, _abi.SENSOR_HEADERS, _abi.SURFACE_HEADERS, _abi.ALIGN_HEADERS, _abi.SHADE_HEADERS)


def test_mesh_shade_abi_exported_and_bound():
    from diff_gaussian_rasterization import _abi
    protos = test_abi._prototypes([HEADER])
    assert list(_abi.SHADE_HEADERS) == [HEADER] and all(HEADER not in t for t in tables()[:-1])
    assert HEADER not in test_abi.ALL_HEADERS
    assert [s[0] for s in _abi.SHADE_HEADERS[HEADER]] == list(protos) == NAMES      # the header's names in the header's order
    assert test_abi.check_header(HEADER) == NAMES      # exported, and bound with the header's type classes
    for name, restype, argtypes in _abi.SHADE_HEADERS[HEADER]:      # _load() bound this table as it binds the other six
        fn = getattr(_abi.lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    bound = [s[0] for t in tables() for table in t.values() for s in table]
    assert sorted(bound) == sorted(set(bound))      # no name twice across the seven tables
    assert protos["hsr_mesh_normals_scratch_bytes"][1:] == ("size_t", ["int"])
    assert protos["hsr_mesh_normals"][1:] == ("int", ["int", "int", FP, IP, VP, "size_t", FP, VP])
    assert protos["hsr_mesh_shade"][1:] == ("int", ["int", "int", FP, IP, "int", "int"] + ["float"] * 4 + [FP, IP, "int", ("pointer", "hsr_shade_job"), VP])
    assert _abi.lib.hsr_mesh_shade.argtypes[10] is _abi.fp      # w2c is a HOST pointer: a ctypes array goes in by address
    assert _abi.lib.hsr_mesh_shade.argtypes[13] is C.POINTER(_abi.hsr_shade_job)


def test_job_struct_and_constants_match_the_header():
    from diff_gaussian_rasterization import _abi
    from hsr_utils import mesh_view
    structs = test_abi._structures([HEADER])
    assert list(structs) == ["hsr_shade_job"]
    assert structs["hsr_shade_job"] == [f[0] for f in _abi.hsr_shade_job._fields_]
    assert structs["hsr_shade_job"] == ["kind", "lit", "normals", "attr", "table", "n", "lo", "hi", "ambient", "albedo", "background", "out"]
    job = _abi.hsr_shade_job
    assert (job.kind.offset, job.lit.offset, job.normals.offset, job.attr.offset, job.table.offset, job.n.offset) == (0, 4, 8, 16, 24, 32)
    assert (job.lo.offset, job.hi.offset, job.ambient.offset, job.albedo.offset, job.background.offset, job.out.offset) == (36, 40, 44, 48, 60, 64)
    assert C.sizeof(job) == 72 and job.albedo.size == 12 and job.background.size == 4
    source = test_abi._source(HEADER)
    for name, value in (("HSR_SHADE_MAX_JOBS", mesh_view.MAX_JOBS), ("HSR_SHADE_SHADED ", mesh_view.SHADED), ("HSR_SHADE_COLOUR ", mesh_view.COLOUR),
                        ("HSR_SHADE_NORMALS", mesh_view.NORMALS), ("HSR_SHADE_LABELS ", mesh_view.LABELS), ("HSR_SHADE_SCALAR ", mesh_view.SCALAR)):
        assert "#define %s %d" % (name, value) in source, name
    assert (mesh_view.SHADED, mesh_view.COLOUR, mesh_view.NORMALS, mesh_view.LABELS, mesh_view.SCALAR) == (R.SHADED, R.COLOUR, R.NORMALS, R.LABELS, R.SCALAR)
    assert mesh_view.MAX_JOBS == 8 and tuple(mesh_view.PICTURES) == tuple(R.KINDS)
    assert "#include \"hsr_mesh_face.h\"" in open(os.path.join(test_abi.ROOT, "hier-slam_amd", "csrc", "hsr_mesh_depth.hip")).read()
    assert "#include \"hsr_mesh_face.h\"" in open(os.path.join(test_abi.ROOT, "hier-slam_amd", "csrc", "hsr_mesh_shade.hip")).read()


def test_names_are_reached_lazily_from_the_package():
    import hsr_utils
    from hsr_utils import mesh_view
    assert tuple(hsr_utils._MESH_VIEW) == tuple(mesh_view.__all__)
    for name in hsr_utils._MESH_VIEW:
        assert getattr(hsr_utils, name) is getattr(mesh_view, name), name
    others = [getattr(hsr_utils, n) for n in dir(hsr_utils) if n.startswith("_") and n.isupper() and n != "_MESH_VIEW" and isinstance(getattr(hsr_utils, n), tuple)]
    assert len(others) >= 13
    assert not set(hsr_utils._MESH_VIEW) & {name for t in others for name in t}
    from hsr_utils import slam
    assert callable(slam.SlamSession.render_mesh)


# ---- refusals: dummy non-device pointers that are never followed ---------------------------------------------------------------------------
W2C = (C.c_float * 16)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1)
P = [4096 * (n + 1) for n in range(10)]      # 16-byte aligned


def normals_call(lib, V=4, F=2, vertices=P[0], faces=P[1], scratch=P[2], scratch_bytes=None, out=P[3]):
    if scratch_bytes is None:
        scratch_bytes = lib.hsr_mesh_normals_scratch_bytes(max(V, 0))
    return lib.hsr_mesh_normals(V, F, vertices, faces, scratch, scratch_bytes, out, None)


NORMALS_REFUSALS = (
    [(o, b"invalid sizes") for o in (dict(V=0), dict(V=-2), dict(F=-1))]
    + [({n: None}, b"are required") for n in ("vertices", "scratch", "out")]
    + [(dict(faces=None), b"faces are required with F > 0")]
    + [(dict(scratch_bytes=0), b"the scratch must hold"), (dict(scratch_bytes=95), b"the scratch must hold")]
    + [(dict(scratch=P[2] + 8), b"16-byte aligned"), (dict(scratch=P[2] + 4), b"16-byte aligned")]
)


@pytest.mark.parametrize("overrides,message", NORMALS_REFUSALS, ids=["%d" % i for i in range(len(NORMALS_REFUSALS))])
def test_normals_refuses_before_any_device_work(overrides, message):
    from diff_gaussian_rasterization import _abi
    rc = normals_call(_abi.lib, **overrides)
    err = _abi.lib.hsr_last_error()
    assert rc == -1 and err.startswith(b"mesh_shade: ") and message in err, (overrides, rc, err)


def shade_call(lib, V=4, F=2, vertices=P[0], faces=P[1], H=6, W=8, fx=8.0, fy=8.0, cx=3.5, cy=2.5, w2c=W2C, face_image=P[2], n_jobs=1, jobs=True,
               **fields):
    from diff_gaussian_rasterization import _abi
    array = (_abi.hsr_shade_job * 8)()
    for k, job in enumerate(array):
        job.kind, job.lit, job.normals, job.attr, job.table, job.n = R.SHADED, 1, P[3], P[4], P[5], 256
        job.lo, job.hi, job.ambient, job.out = 0.0, 1.0, 0.25, P[6] + 4096 * k
    for name, value in fields.items():      # a field of the LAST job of the call: the jobs before it are fine
        setattr(array[max(min(n_jobs, 8), 1) - 1], name, value)
    return lib.hsr_mesh_shade(V, F, vertices, faces, H, W, fx, fy, cx, cy, w2c, face_image, n_jobs, array if jobs else None, None)


SHADE_REFUSALS = (
    [(o, b"invalid sizes") for o in (dict(V=0), dict(V=-2), dict(F=-1))]
    + [(o, b"invalid image size") for o in (dict(H=0), dict(W=0), dict(H=16385), dict(W=16385), dict(H=-4))]
    + [({n: v}, b"must be finite and not zero") for n in ("fx", "fy") for v in (0.0, NAN, INF, -INF)]
    + [({n: v}, b"cx and cy finite") for n in ("cx", "cy") for v in (NAN, INF)]
    + [({n: None}, b"are required") for n in ("w2c", "face_image")]
    + [({n: None}, b"are required with F > 0") for n in ("vertices", "faces")]
    + [(o, b"n_jobs must be 1..8") for o in (dict(n_jobs=0), dict(n_jobs=9), dict(n_jobs=-1), dict(jobs=False))]
    + [(dict(kind=v, n_jobs=n), b"unknown kind") for v in (-1, 5) for n in (1, 3, 8)]
    + [(dict(out=None, kind=kind), b"NULL out, attr or table") for kind in range(5)]
    + [(dict(attr=None, kind=kind), b"NULL out, attr or table") for kind in (R.COLOUR, R.LABELS, R.SCALAR)]
    + [(dict(table=None, kind=kind, n_jobs=2), b"NULL out, attr or table") for kind in (R.LABELS, R.SCALAR)]
    + [(dict(kind=R.LABELS, n=v), b"LABELS at least 1") for v in (0, -3)]
    + [(dict(kind=R.SCALAR, n=v), b"SCALAR takes 256") for v in (255, 257, 0)]
    + [(dict(kind=R.SCALAR, lo=lo, hi=hi), b"hi - lo must be finite and positive") for lo, hi in ((1.0, 1.0), (2.0, 1.0), (0.0, INF), (NAN, 1.0), (-3e38, 3e38))]
    + [(dict(ambient=v, kind=kind), b"ambient must be in [0, 1]") for v in (-0.01, 1.01, NAN, INF) for kind in (R.SHADED, R.NORMALS)]
)


@pytest.mark.parametrize("overrides,message", SHADE_REFUSALS, ids=["%d" % i for i in range(len(SHADE_REFUSALS))])
def test_shade_refuses_before_any_device_work(overrides, message):
    from diff_gaussian_rasterization import _abi
    rc = shade_call(_abi.lib, **overrides)
    err = _abi.lib.hsr_last_error()
    assert rc == -1 and err.startswith(b"mesh_shade: ") and message in err, (overrides, rc, err)


def test_fields_a_kind_does_not_name_are_not_checked():
    """a NULL attr or table, an n of 0 and an empty range refuse nothing where the kind does not read them: the call gets as far as the
    next refusal, the NULL out of the job after it"""
    from diff_gaussian_rasterization import _abi
    for kind, fields in ((R.SHADED, dict(attr=None, table=None, n=0, lo=1.0, hi=1.0)), (R.NORMALS, dict(attr=None, table=None, n=0)),
                         (R.COLOUR, dict(table=None, n=0, lo=1.0, hi=1.0)), (R.LABELS, dict(lo=1.0, hi=1.0, n=1))):
        array = (_abi.hsr_shade_job * 2)()
        array[0].kind, array[0].out, array[0].attr, array[0].table, array[0].n, array[0].ambient = kind, P[6], P[4], P[5], 256, 1.0
        for name, value in fields.items():
            setattr(array[0], name, value)
        array[1].kind, array[1].out = R.SHADED, None
        rc = _abi.lib.hsr_mesh_shade(4, 2, P[0], P[1], 6, 8, 8.0, 8.0, 3.5, 2.5, W2C, P[2], 2, array, None)
        assert rc == -1 and _abi.lib.hsr_last_error().startswith(b"mesh_shade: job 1 "), (kind, _abi.lib.hsr_last_error())


def test_scratch_bytes_is_monotone_and_zero_for_a_negative_count():
    from diff_gaussian_rasterization import _abi
    size = _abi.lib.hsr_mesh_normals_scratch_bytes
    assert size(-1) == 0 and size(-2 ** 31) == 0 and size(0) == 0
    assert [size(V) for V in (1, 2, 3, 4)] == [32, 48, 80, 96]      # 24 bytes a vertex, rounded up to 16
    sizes = [size(V) for V in (0, 1, 2, 5, 1000, 10 ** 6, 2 ** 31 - 1)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes) and all(s % 16 == 0 for s in sizes)
    assert sizes[-1] == 24 * (2 ** 31 - 1) + 8      # past 2^31: the size is a size_t


# ---- orbit views --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(elevation_deg=0.0), dict(elevation_deg=-40.0, distance=2.5), dict(up=(0.0, 0.0, 2.0)),
                                dict(elevation_deg=90.0), dict(up=(1.0, 1.0, 0.2), elevation_deg=65.0)],
                         ids=["default", "level", "below", "z_up", "overhead", "tilted_up"])
def test_orbit_views_follow_the_stated_construction(kw):
    from hsr_utils import mesh_view
    lo, hi, n = np.array([-1.0, -0.5, 0.25]), np.array([2.0, 1.5, 3.0]), 7
    views = mesh_view.orbit_views(lo, hi, n, **kw)
    assert isinstance(views, np.ndarray) and views.dtype == np.float32 and views.shape == (n, 4, 4)
    assert np.array_equal(views, mesh_view.orbit_views(lo.tolist(), hi.tolist(), n, **kw))      # the same views from the same arguments
    assert mesh_view.orbit_views(lo, hi, 0).shape == (0, 4, 4)
    eyes = []
    for i, view in enumerate(views.astype(np.float64)):
        eye, centre, distance, u = R.orbit_view(lo, hi, n, i, **kw)
        rot = view[:3, :3]
        assert np.array_equal(view[3], [0, 0, 0, 1])
        assert np.abs(rot @ rot.T - np.eye(3)).max() <= 1e-6 and abs(np.linalg.det(rot) - 1) <= 1e-6
        got_eye = -rot.T @ view[:3, 3]
        assert np.abs(got_eye - eye).max() <= 1e-5 * max(1.0, distance)
        assert abs(np.linalg.norm(got_eye - centre) - distance) <= 1e-5 * distance      # every camera at the stated distance
        p = rot @ centre + view[:3, 3]      # the centre lies on the viewing axis: it projects to the principal point
        assert p[2] > 0 and abs(p[0]) <= 1e-5 * distance and abs(p[1]) <= 1e-5 * distance and abs(p[2] - distance) <= 1e-5 * distance
        if np.linalg.norm(np.cross(rot[2], u)) >= 1e-3:      # up stays up in the image: image-down has no part along up's side
            assert rot[1] @ u < 0 and abs(rot[0] @ u) <= 1e-6
        eyes.append(got_eye)
    if kw.get("elevation_deg") != 90.0:
        assert len({tuple(np.round(e, 4)) for e in eyes}) == n      # n different places on the circle
    if not kw:
        assert abs(distance - 1.5 * np.linalg.norm(hi - lo)) < 1e-12 and np.array_equal(u, [0, -1, 0])
        assert all(e[1] < centre[1] for e in eyes)      # above the box in a world whose y points down


def test_orbit_views_host_errors():
    from hsr_utils import mesh_view
    with pytest.raises(ValueError, match="number of views must be >= 0"):
        mesh_view.orbit_views([0, 0, 0], [1, 1, 1], -1)
    with pytest.raises(ValueError, match="distance must be finite and positive"):
        mesh_view.orbit_views([0, 0, 0], [0, 0, 0], 3)
    with pytest.raises(ValueError, match="up must not be zero"):
        mesh_view.orbit_views([0, 0, 0], [1, 1, 1], 3, up=(0, 0, 0))
    with pytest.raises(ValueError, match="the box must be finite"):
        mesh_view.orbit_views([0, 0, NAN], [1, 1, 1], 3)


# ---- the restatement against analysis -----------------------------------------------------------------------------------------------------
def test_restated_normals_of_a_sphere_point_outwards():
    """An octahedron subdivided twice onto the unit sphere, 128 faces: the area-weighted normal of a vertex against its radial
    direction.  The discretisation decides the angle, not the arithmetic: measured on this mesh in plain float64 (normals64) the largest
    angle is 9.782e-2 rad (5.6 degrees, at the vertices where the subdivision's faces are least alike; 0 at the octahedron's own six), and the bound is
    twice that.  The
    restatement (float32 crosses, 2^40 fixed point) must stay within it and within 1e-6 of the float64 normals: a cross of this mesh has
    components below 0.2, so its float32 rounding is below 2e-8 and the fixed point's below 1e-12 a face."""
    vertices, faces = R.sphere(2)
    assert faces.shape == (128, 3) and vertices.shape == (66, 3)
    radial = vertices.astype(np.float64) / np.linalg.norm(vertices.astype(np.float64), axis=1, keepdims=True)
    for tri in faces:      # wound outwards
        assert R.face_cross(vertices, tri) @ vertices[tri].mean(axis=0) > 0
    n64 = R.normals64(vertices, faces)
    angle64 = np.arccos(np.clip((n64 * radial).sum(1), -1, 1))
    print("float64: largest angle to the radial direction %.4e rad" % angle64.max())
    assert 9.7e-2 < angle64.max() < 9.9e-2      # the figure the docstring states
    n = R.normals(vertices, faces)
    assert n.dtype == np.float32 and n.shape == (66, 3)
    angle = np.arccos(np.clip((n.astype(np.float64) * radial).sum(1), -1, 1))
    print("restatement: largest angle %.4e rad; largest difference from float64 %.3e" % (angle.max(), np.abs(n - n64).max()))
    assert angle.max() <= 2 * 9.782e-2
    assert np.abs(n - n64).max() <= 1e-6 and np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() <= 1e-6


def test_restated_normals_take_no_part_clauses_and_order():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [5, 5, 5]], np.float32)
    one = R.normals(v, [[0, 1, 2]])
    assert np.array_equal(one, np.array([[0, 0, 1]] * 3 + [[0, 0, 0]] * 2, np.float32))      # an unused vertex: zeros
    for bad in ([0, 1, 5], [-1, 1, 2], [0, 0, 1]):      # an index of V, of -1, a face without area
        assert np.array_equal(R.normals(v, [[0, 1, 2], bad]), one)
    huge = v.copy()
    huge[4] = [1e30, 0, 0]
    assert np.array_equal(R.normals(huge, [[0, 1, 2], [0, 4, 3]])[:3], one[:3])      # its cross is not finite
    big = v * np.float32(300)      # a cross of 90000 >= 2^16
    assert (R.normals(big, [[0, 1, 2]]) == 0).all() and (R.normals(v * np.float32(255), [[0, 1, 2]])[:3] == [0, 0, 1]).all()
    vertices, faces = R.fan(200)
    a, b = R.normals(vertices, faces), R.normals(vertices, faces[np.random.default_rng(0).permutation(len(faces))])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))      # integer sums: any order of the faces, the same bits
    assert np.array_equal(R.normals(v, np.zeros((0, 3), np.int32)), np.zeros((5, 3), np.float32))


def plane_terms():
    vertices, faces = D.tilted_plane(0)
    depth, face = D.render(vertices, faces, np.eye(4), D.PLANE_K, D.PLANE_H, D.PLANE_W)
    return vertices, faces, depth, face, R.pixel_terms(vertices, faces, np.eye(4), D.PLANE_K, D.PLANE_H, D.PLANE_W, face)


def test_restated_weights_sum_to_one_and_reproduce_the_depth():
    """at every hit pixel of the tilted plane: z is the depth image's own number bit for bit (the same det / s), the three weights
    sum to 1 within 4 ulp of 1 (three correctly rounded quotients of one s: each is off by half an ulp of a number <= 1, and two additions
    round once more each), no weight lies outside [0, 1] by more than that, and the hit point p is on the analytic plane"""
    vertices, faces, depth, face, t = plane_terms()
    hit = face.reshape(-1) >= 0
    assert hit.sum() > 3000 and np.array_equal(t["hit"], hit)
    assert np.array_equal(t["z"][hit].view(np.uint32), depth.reshape(-1)[hit].view(np.uint32))
    b = t["b"][hit]
    total = (b[:, 0] + b[:, 1]) + b[:, 2]
    ulp = float(np.finfo(np.float32).eps)
    print("largest |sum of the weights - 1|: %.3e (%.2f ulp)" % (np.abs(total - 1).max(), np.abs(total - 1).max() / ulp))
    assert np.abs(total.astype(np.float64) - 1).max() <= 4 * ulp
    assert b.min() >= -4 * ulp and b.max() <= 1 + 4 * ulp
    p = t["p"][hit].astype(np.float64)
    assert np.abs(p[:, 2] - (3 + 0.4 * p[:, 0] - 0.3 * p[:, 1])).max() <= 4 * 2.87e-6 * p[:, 2].max()      # mesh_depth's measured figure
    corners = D.camera_points(vertices, np.eye(4)).astype(np.float64)[t["idx"][hit]]      # [n, corner, 3]
    mix = (b[:, :, None].astype(np.float64) * corners).sum(1)
    assert np.abs(mix - p).max() <= 2e-5      # the weights are barycentric in 3D: they mix the corners into the hit point
    assert (np.abs(np.linalg.norm(t["v"][hit].astype(np.float64), axis=1) - 1) <= 1e-6).all()
    assert ((t["v"][hit].astype(np.float64) * p).sum(1) < 0).all()      # the view vector points back at the camera


def test_restated_colour_linear_in_position_interpolates_exactly():
    """a vertex colour that is linear in world position, c = 128 + 8 x - 6 y + 4 z in the first channel (other coefficients a channel),
    quantised to uint8 at the vertices: the unlit COLOUR picture at a hit pixel is that function at the hit point, to the vertex
    quantisation (half a grey level), the interpolation's float32 error and the byte rounding (half a level): 1.01 levels in all"""
    vertices, faces, depth, face, t = plane_terms()
    coef = np.array([[128, 8, -6, 4], [120, -5, 9, 3], [100, 4, 6, 8]], np.float64)
    value = lambda p: coef[:, 0] + p @ coef[:, 1:].T
    rgb = np.rint(value(vertices.astype(np.float64))).astype(np.int64)
    assert rgb.min() >= 0 and rgb.max() <= 255 and rgb.max() - rgb.min() > 100
    picture = R.shade(vertices, faces, np.eye(4), D.PLANE_K, D.PLANE_H, D.PLANE_W, face, [R.job("colour", attr=rgb.astype(np.uint8), lit=False)], terms=t)[0]
    hit = t["hit"]
    want = value(t["p"][hit].astype(np.float64))
    got = picture.reshape(-1, 3)[hit].astype(np.float64)
    print("largest difference from the linear colour: %.3f grey levels" % np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1.01
    assert (picture.reshape(-1, 3)[~hit] == 255).all() and (~hit).sum() > 0      # the background elsewhere
    lit = R.shade(vertices, faces, np.eye(4), D.PLANE_K, D.PLANE_H, D.PLANE_W, face, [R.job("colour", attr=rgb.astype(np.uint8), lit=True)], terms=t)[0]
    assert (lit.reshape(-1, 3)[hit].astype(int) <= got + 0.5).all() and (lit.reshape(-1, 3)[hit] < got - 1).any()      # shade <= 1 darkens


def test_restated_shading_of_the_plane():
    """the plane's flat normal is one direction whatever the winding (two-sided shading turns it to the camera), the NORMALS picture is
    blue-ish, the shade is ambient + (1 - ambient) |n . v| of the analytic normal within 2 grey levels, and a smooth picture with the
    plane's own vertex normals equals the flat one within a level (every vertex normal is the plane's)"""
    vertices, faces, depth, face, t = plane_terms()
    hit = t["hit"]
    n = R.shading_normal(t, np.eye(4), None)[hit].astype(np.float64)
    analytic = np.array([0.4, -0.3, -1.0]) / np.linalg.norm([0.4, -0.3, -1.0])      # towards the camera (negative z)
    assert np.abs(n - analytic).max() <= 1e-5
    args = (vertices, faces, np.eye(4), D.PLANE_K, D.PLANE_H, D.PLANE_W, face)
    vn = R.normals(vertices, faces)      # windings are random: the sum at a vertex is not the plane's normal, but a tensor of them is
    plane_normals = np.tile(analytic.astype(np.float32), (len(vertices), 1))
    flat, smooth, colours = R.shade(*args, [R.job("shaded"), R.job("shaded", normals=plane_normals), R.job("normals")], terms=t)
    ndv = np.abs((t["v"][hit].astype(np.float64) * analytic).sum(1))
    want = 255 * 0.8 * (0.25 + 0.75 * ndv)
    assert np.abs(flat.reshape(-1, 3)[hit].astype(np.float64) - want[:, None]).max() <= 1.0
    assert np.abs(flat.astype(int) - smooth.astype(int)).max() <= 1
    blue = colours.reshape(-1, 3)[hit].astype(int)
    assert (blue[:, 2] > 200).all() and (np.abs(blue - np.rint(255 * (np.array([0.4, 0.3, 1.0]) / np.linalg.norm([0.4, 0.3, 1.0]) * 0.5 + 0.5))) <= 1).all()
    assert vn.shape == vertices.shape


def test_restated_byte_rule_and_table_kinds():
    assert R.code(np.array([NAN, -1, 0, 0.5 / 255, 1.5 / 255, 2.5 / 255, 1, 2, INF, -INF], np.float32)).tolist()[:3] == [0, 0, 0]
    assert R.code(np.array([1, 2, INF], np.float32)).tolist() == [255, 255, 255] and R.code(np.float32(-INF)) == 0
    halves = R.code(np.array([0.5, 1.5, 2.5, 3.5], np.float32) / np.float32(255))      # whichever side the quotient's rounding falls, within one
    assert all(abs(int(h) - w) <= 1 for h, w in zip(halves, (0, 2, 2, 4)))
    v = np.array([[-1, -1, 2], [1, -1, 2], [0, 1, 2]], np.float32)
    k = np.array([[8.0, 0, 3.5], [0, 8.0, 2.5], [0, 0, 1]])
    face = D.render(v, [[0, 1, 2]], np.eye(4), k, 6, 8)[1]
    table, jet = R.table(4), R.table(256, 1)
    labels = np.array([3, 4, -1], np.int32)      # n - 1, n and -1 for a table of 4
    scalar = np.array([0.0, 1.0, NAN], np.float32)
    lab, sca = R.shade(v, [[0, 1, 2]], np.eye(4), k, 6, 8, face, [R.job("labels", attr=labels, table=table, lit=False),
                                                                     R.job("scalar", attr=scalar, table=jet, lo=0.0, hi=1.0, lit=False)])
    hit = face >= 0
    seen = {tuple(c) for c in lab[hit].tolist()}
    assert seen == {tuple(table[3].tolist()), (0, 0, 0)} and (lab[~hit] == 255).all()      # corner A's label through the table; B's and C's black
    assert (sca[hit] == jet[0]).all()      # a NaN corner makes the interpolated scalar NaN: index 0


# ---- the tool -----------------------------------------------------------------------------------------------------------------------------
def test_tool_has_its_options():
    source = open(os.path.join(test_abi.ROOT, "tools", "render_mesh.py")).read()
    for option in ("mesh_ply", "out_dir", "--params", "--every", "--orbit", "--pictures", "--gt", "--flat", "--size"):
        assert "\"%s\"" % option in source, option
    assert "shaded,colour,labels,normals,scalar" in source and "render_mesh_run" in source and "render_mesh_views" in source
    bench = open(os.path.join(test_abi.ROOT, "tools", "bench_mesh_view.py")).read()
    assert "hsr_mesh_shade" in bench and "index_add_" in bench and "vertex_normals" in bench
