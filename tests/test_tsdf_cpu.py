"""CPU suite for the mesh of a finished run: the numpy restatement of include/ext/hsr_tsdf.h (tests/tsdf_ref.py) against what a mesh must
be — closed, manifold, outward, near the surface — on an analytic sphere and at the grid's edges; the prototypes of the header (their
names and type classes; tests/test_abi.py checks that they are exported and bound with the header's types); every refusal of the header with
dummy pointers; the PLY file, the bounds and the host argument errors of hsr_utils.mesh.  Nothing here launches: there is no GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import test_abi
import tsdf_ref as R

EXT_HEADER = "ext/hsr_tsdf.h"
NAMES = ["hsr_tsdf_integrate", "hsr_tsdf_count", "hsr_tsdf_faces", "hsr_tsdf_vertices"]
FP, VP, IP, LP = ("pointer", "float"), ("pointer", "void"), ("pointer", "int"), ("pointer", "int64_t")

SPHERE_DIMS, SPHERE_H, SPHERE_C, SPHERE_R, SPHERE_TRUNC = (21, 19, 17), 0.1, (1.013, 0.887, 0.821), 0.55, 0.3


def test_tsdf_abi_exported_and_bound():
    from diff_gaussian_rasterization import _abi
    protos = test_abi._prototypes([EXT_HEADER])
    assert [s[0] for s in _abi.HEADERS[EXT_HEADER]] == list(protos) == NAMES
    assert protos["hsr_tsdf_integrate"][1:] == ("int", ["int"] * 3 + ["float"] * 6 + ["int", "int"] + ["float"] * 4 + [FP, FP, FP, LP, FP, "float",
                                                        "float"] + [FP] * 5 + [IP, VP])
    assert protos["hsr_tsdf_count"][1:] == ("int", ["int"] * 3 + [FP, FP, IP, VP])
    assert protos["hsr_tsdf_faces"][1:] == ("int", ["int"] * 3 + [FP, FP, LP, "size_t", LP, VP])
    assert protos["hsr_tsdf_vertices"][1:] == ("int", ["int"] * 3 + ["float"] * 4 + ["size_t", LP, FP, FP, FP, IP, FP, ("pointer", "uint8_t"), IP, VP])
    # w2c is the one HOST pointer: bound as a float pointer, so that a ctypes array goes in by address
    assert _abi.lib.hsr_tsdf_integrate.argtypes[15] is _abi.fp
    from hsr_utils import mesh
    assert "#define HSR_TSDF_MAX_IMAGE_SIDE 16384" in test_abi._source(EXT_HEADER) and mesh.MAX_IMAGE_SIDE == 16384


def test_names_are_reached_lazily_from_the_package():
    import hsr_utils
    from hsr_utils import mesh
    assert set(hsr_utils._MESH) == set(mesh.__all__)
    for name in hsr_utils._MESH:
        assert getattr(hsr_utils, name) is getattr(mesh, name), name
    assert callable(hsr_utils.SlamSession.export_mesh)


# ---- the restatement: what a mesh must be ---------------------------------------------------------------------------------------------------
def test_the_tetrahedra_tile_the_cube_with_the_stated_orientations():
    assert tuple(R.tet_orientation(t) for t in R.TETS) == R.TET_SIGN
    corner = lambda c: np.array([(c >> a) & 1 for a in range(3)], np.float64)
    volume = sum(abs(np.linalg.det(np.stack([corner(t[q]) - corner(t[0]) for q in (1, 2, 3)]))) / 6 for t in R.TETS)
    assert abs(volume - 1.0) < 1e-12
    for t in R.TETS:      # nested corner sets: every edge runs from a point to that point plus an offset in {0,1}^3
        assert all(t[a] & t[b] == t[a] for a in range(4) for b in range(a, 4))


@pytest.fixture(scope="module")
def sphere():
    vol = R.sphere_volume(SPHERE_DIMS, SPHERE_H, SPHERE_C, SPHERE_R, SPHERE_TRUNC)
    return vol, R.extract(vol)


def check_sphere_mesh(pos, faces):
    """the conditions of the analytic sphere, for the restatement here and for the device's mesh in tests/test_gpu_tsdf.py"""
    closed, euler = R.topology(faces)
    assert closed, "an edge that is not in exactly two faces, once in each direction"
    assert euler == 2, euler
    assert len(np.unique(faces)) == len(pos)
    assert R.signed_volume(pos, faces) > 0
    # derivable: the zero of a linear interpolant of a 1-Lipschitz function lies on an edge no longer than the cube's diagonal
    off = np.abs(np.linalg.norm(np.asarray(pos, np.float64) - np.array(SPHERE_C), axis=1) - SPHERE_R)
    assert off.max() <= SPHERE_H * np.sqrt(3.0), off.max()
    return off.max()


def test_sphere_mesh_is_closed_manifold_outward_and_near_the_sphere(sphere):
    vol, (pos, faces, rgb, labels, keys) = sphere
    assert rgb is None and labels is None and pos.dtype == np.float32 and faces.dtype == np.int32
    assert len(faces) > 500 and (np.diff(keys) > 0).all()
    check_sphere_mesh(pos, faces)
    volume = R.signed_volume(pos, faces)
    assert abs(volume - 4 / 3 * np.pi * SPHERE_R ** 3) < 0.1 * volume      # and it is the sphere's, within a voxel layer
    assert np.array_equal(R.cube_counts(*SPHERE_DIMS, vol.tsdf, vol.weight).sum(), len(faces))
    # the normals point away from the centre on average per face
    p = pos.astype(np.float64)[faces]
    normal = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    outward = np.einsum("ij,ij->i", normal, p.mean(axis=1) - np.array(SPHERE_C))
    assert (outward >= -1e-12).all()


def _cube(inside_corners, weight=None):
    vol = R.Volume((0.0, 0.0, 0.0), (2, 2, 2), 1.0, 1.0, 64.0, color=False)
    vol.weight = np.ones(8, np.float32) if weight is None else np.asarray(weight, np.float32)
    vol.tsdf = np.full(8, 0.5, np.float32)
    vol.tsdf[list(inside_corners)] = -0.5
    return vol


def test_grid_edges():
    one = R.Volume((0.0, 0.0, 0.0), (1, 1, 1), 1.0, 1.0, 64.0, color=False)
    one.tsdf[:], one.weight[:] = -1, 1
    pos, faces, _rgb, _labels, keys = R.extract(one)
    assert pos.shape == (0, 3) and faces.shape == (0, 3) and keys.size == 0 and R.cube_counts(1, 1, 1, one.tsdf, one.weight).tolist() == [0]
    for dims in ((5, 1, 1), (1, 4, 3), (3, 3, 1)):      # a flat grid has no cube
        flat = R.Volume((0.0, 0.0, 0.0), dims, 1.0, 1.0, 64.0, color=False)
        flat.tsdf[::2], flat.weight[:] = -1, 1
        assert R.extract(flat)[1].shape == (0, 3)
    # one corner inside: the fan of the tetrahedra that hold it — all six at corners 0 and 7, two at the others
    for corner, n in zip(range(8), (6, 2, 2, 2, 2, 2, 2, 6)):
        vol = _cube([corner])
        pos, faces, _rgb, _labels, keys = R.extract(vol)
        assert len(faces) == n and R.cube_counts(2, 2, 2, vol.tsdf, vol.weight).tolist() == [n] + [0] * 7
        c = np.array([(corner >> a) & 1 for a in range(3)], np.float64)
        assert np.allclose(np.linalg.norm(pos - c, axis=1), 0.5 * np.linalg.norm(np.round(2 * (pos - c)), axis=1))      # every vertex halfway along an edge at the corner
        p = pos.astype(np.float64)[faces]
        normal = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        assert (np.einsum("ij,ij->i", normal, p.mean(axis=1) - c) > 0).all(), corner      # away from the inside corner
    vol = _cube([0])
    pos, faces, _rgb, _labels, keys = R.extract(vol)
    assert keys.tolist() == [1, 2, 3, 4, 5, 6, 7] and (faces == 6).any(axis=1).all()      # the seven edges at point 0; all six share the diagonal
    directed = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    assert len(np.unique(directed, axis=0)) == 18      # no directed edge twice: the fan is consistently oriented
    # seven corners inside: the same fan, turned over
    pos7, faces7, _rgb, _labels, keys7 = R.extract(_cube(range(1, 8)))
    assert np.array_equal(keys7, keys) and np.array_equal(R.canonical_faces(faces7), R.canonical_faces(faces[:, ::-1]))
    # an exact zero is outside
    zero = _cube([])
    zero.tsdf[0] = 0.0
    assert R.extract(zero)[1].shape == (0, 3)
    zero.tsdf[0] = -0.0
    assert R.extract(zero)[1].shape == (0, 3)


def test_a_cube_with_an_unobserved_point_gives_nothing():
    for corner in range(8):
        weight = np.ones(8, np.float32)
        weight[corner] = 0
        vol = _cube([0, 3, 5], weight)
        assert R.extract(vol)[1].shape == (0, 3) and not R.cube_counts(2, 2, 2, vol.tsdf, vol.weight).any()
    weight = np.ones(8, np.float32)
    weight[6] = np.nan      # not > 0
    assert R.extract(_cube([0], weight))[1].shape == (0, 3)
    assert len(R.extract(_cube([0, 3, 5]))[1]) > 0


def test_two_inside_quads_split_along_the_smallest_key():
    for a in range(8):
        for b in range(a + 1, 8):
            vol = _cube([a, b])
            pos, faces, _rgb, _labels, keys = R.extract(vol)
            closed_dir = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
            assert len(np.unique(closed_dir, axis=0)) == len(closed_dir), (a, b)      # consistently oriented
            p = pos.astype(np.float64)[faces]
            normal = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
            inside = np.array([[(c >> q) & 1 for q in range(3)] for c in (a, b)], np.float64)
            # every face looks away from the inside: the segment between the two corners where a tetrahedron edge joins them (nested
            # corner sets), else the nearer corner
            centre = p.mean(axis=1)
            if a & b == a:
                along = np.clip((centre - inside[0]) @ (inside[1] - inside[0]) / np.sum((inside[1] - inside[0]) ** 2), 0, 1)
                near = inside[0] + along[:, None] * (inside[1] - inside[0])
            else:
                near = inside[np.argmin(np.linalg.norm(centre[:, None] - inside[None], axis=2), axis=1)]
            assert (np.einsum("ij,ij->i", normal, centre - near) > 0).all(), (a, b)


def test_integrate_restatement_on_a_wall():
    """a wall at z = 1 seen from the origin: tsdf = min(1, (1 - z) / trunc) in front of -trunc, nothing behind it, colours in the band"""
    vol = R.Volume((-0.2, -0.2, 0.5), (5, 5, 11), 0.1, 0.25, 64.0, color=True, labels=True)
    H, W = 30, 40
    k = np.array([[30.0, 0, 19.5], [0, 30.0, 14.5], [0, 0, 1]])
    depth = np.ones((H, W), np.float32)
    image = np.stack([np.full((H, W), v, np.float32) for v in (0.25, 0.5, 0.75)])
    labels = np.full((H, W), 70000, np.int64)
    R.integrate(vol, depth, np.eye(4), k, image=image, labels=labels)
    _i, _j, kk = vol.ijk()
    z = np.float32(0.5) + np.float32(0.1) * kk.astype(np.float32)
    sdf = np.float32(1) - z
    seen = ~(sdf < -np.float32(0.25))
    assert np.array_equal(vol.weight, seen.astype(np.float32))
    assert np.array_equal(vol.tsdf[seen], np.fmin(np.float32(1), sdf / np.float32(0.25))[seen]) and (vol.tsdf[~seen] == 1).all()
    band = seen & (np.abs(sdf) <= np.float32(0.25))
    assert band.any() and (~band).any() and np.array_equal(vol.cweight, band.astype(np.float32))
    assert (vol.color[:, band] == np.array([[0.25], [0.5], [0.75]], np.float32)).all() and not vol.color[:, ~band].any()
    assert (vol.label[band] == 70000).all() and (vol.label[~band] == -1).all() and np.array_equal(vol.best[band], np.abs(sdf)[band])
    pos, faces, rgb, lab, _keys = R.extract(vol)
    assert len(faces) > 0 and np.allclose(pos[:, 2], 1.0, atol=1e-6) and (rgb == np.array([64, 128, 191], np.uint8)).all() and (lab == 70000).all()
    # a second, identical view: the running means stay, the weights count
    again = R.integrate(vol.copy(), depth, np.eye(4), k, image=image, labels=labels)
    assert np.array_equal(again.weight, 2 * vol.weight) and np.allclose(again.tsdf, vol.tsdf, atol=1e-6) and np.array_equal(again.label, vol.label)


# ---- refusals: dummy non-device pointers that are never followed -------------------------------------------------------------------------
W2C = (C.c_float * 16)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1)
INTEGRATE_POINTERS = ("depth", "image", "labels", "opacity", "tsdf", "weight", "color", "cweight", "best", "label")


def integrate_call(lib, X=4, Y=3, Z=2, h=0.1, trunc=0.3, max_weight=64.0, H=6, W=8, w2c=W2C, **pointers):
    args = {name: 4096 * (n + 1) for n, name in enumerate(INTEGRATE_POINTERS)}
    args.update(pointers)
    a = [args[n] for n in INTEGRATE_POINTERS]
    return lib.hsr_tsdf_integrate(X, Y, Z, 0.0, 0.0, 0.0, h, trunc, max_weight, H, W, 8.0, 8.0, 3.5, 2.5, w2c, a[0], a[1], a[2], a[3], 0.5, 0.0,
                                  *a[4:], None)


NAN, INF = float("nan"), float("inf")
INTEGRATE_REFUSALS = (
    [(dict(X=0), b"invalid volume X=0"), (dict(Y=-1), b"invalid volume"), (dict(Z=0), b"invalid volume X=4 Y=3 Z=0"),
     (dict(X=2048, Y=1024, Z=1024), b"X*Y*Z <= 2^31-1"), (dict(X=65536, Y=65536, Z=1), b"invalid volume"),
     (dict(X=2 ** 31 - 1, Y=2 ** 31 - 1, Z=2 ** 31 - 1), b"invalid volume")]
    + [({name: v}, b"must be finite and positive") for name in ("h", "trunc", "max_weight") for v in (0.0, -1.0, NAN, INF, -INF)]
    + [(dict(H=0), b"invalid image size H=0 W=8"), (dict(W=0), b"invalid image size"), (dict(H=16385), b"invalid image size"),
       (dict(W=16385), b"(1..16384)"), (dict(H=-4), b"invalid image size")]
    + [({name: None}, b"are required") for name in ("w2c", "depth", "tsdf", "weight")]
    + [(dict(color=None), b"come in pairs"), (dict(cweight=None), b"come in pairs"), (dict(best=None), b"come in pairs"),
       (dict(label=None), b"come in pairs"), (dict(color=None, cweight=None), b"image needs color / cweight"),
       (dict(best=None, label=None), b"labels need best / label")]
)


@pytest.mark.parametrize("overrides,message", INTEGRATE_REFUSALS, ids=["%d" % i for i in range(len(INTEGRATE_REFUSALS))])
def test_integrate_refuses_before_any_device_work(overrides, message):
    from diff_gaussian_rasterization import _abi
    rc = integrate_call(_abi.lib, **overrides)
    err = _abi.lib.hsr_last_error()
    assert rc == -1 and err.startswith(b"tsdf_integrate: ") and message in err, (overrides, rc, err)


def count_call(lib, X=4, Y=3, Z=2, tsdf=4096, weight=8192, out_counts=12288):
    return lib.hsr_tsdf_count(X, Y, Z, tsdf, weight, out_counts, None)


def faces_call(lib, X=4, Y=3, Z=2, tsdf=4096, weight=8192, offsets=12288, T=5, out_keys=16384):
    return lib.hsr_tsdf_faces(X, Y, Z, tsdf, weight, offsets, T, out_keys, None)


def vertices_call(lib, X=4, Y=3, Z=2, h=0.1, V=5, keys=4096, tsdf=8192, color=12288, cweight=16384, label=20480, out_vertices=24576,
                  out_rgb=28672, out_labels=32768):
    return lib.hsr_tsdf_vertices(X, Y, Z, 0.0, 0.0, 0.0, h, V, keys, tsdf, color, cweight, label, out_vertices, out_rgb, out_labels, None)


SIZES = [dict(X=0), dict(Y=0), dict(Z=-3), dict(X=2048, Y=1024, Z=1024)]
SURFACE_REFUSALS = (
    [(count_call, b"tsdf_count: ", s, b"invalid volume") for s in SIZES]
    + [(count_call, b"tsdf_count: ", {n: None}, b"are required") for n in ("tsdf", "weight", "out_counts")]
    + [(faces_call, b"tsdf_faces: ", s, b"invalid volume") for s in SIZES]
    + [(faces_call, b"tsdf_faces: ", {n: None}, b"are required") for n in ("tsdf", "weight", "offsets", "out_keys")]
    + [(faces_call, b"tsdf_faces: ", dict(T=24 * 12 + 1), b"more than twelve triangles per point")]
    + [(vertices_call, b"tsdf_vertices: ", s, b"invalid volume") for s in SIZES]
    + [(vertices_call, b"tsdf_vertices: ", dict(h=v), b"h must be finite and positive") for v in (0.0, -0.1, NAN, INF)]
    + [(vertices_call, b"tsdf_vertices: ", dict(V=2 ** 31), b"V <= 2^31-1")]
    + [(vertices_call, b"tsdf_vertices: ", {n: None}, b"are required with V > 0") for n in ("keys", "tsdf", "out_vertices")]
    + [(vertices_call, b"tsdf_vertices: ", {n: None}, b"out_rgb needs color and cweight") for n in ("color", "cweight")]
    + [(vertices_call, b"tsdf_vertices: ", dict(label=None), b"out_labels needs label")]
)


@pytest.mark.parametrize("call,prefix,overrides,message", SURFACE_REFUSALS, ids=["%d" % i for i in range(len(SURFACE_REFUSALS))])
def test_surface_entry_points_refuse_before_any_device_work(call, prefix, overrides, message):
    from diff_gaussian_rasterization import _abi
    rc = call(_abi.lib, **overrides)
    err = _abi.lib.hsr_last_error()
    assert rc == -1 and err.startswith(prefix) and message in err, (overrides, rc, err)


def test_nothing_to_do_launches_nothing():
    """T == 0 and V == 0 return before any device work, whatever the output pointers are"""
    from diff_gaussian_rasterization import _abi
    assert faces_call(_abi.lib, T=0, out_keys=None) == 0
    assert vertices_call(_abi.lib, V=0, keys=None, out_vertices=None, out_rgb=None, out_labels=None) == 0


# ---- the file and the bounds --------------------------------------------------------------------------------------------------------------
def test_mesh_ply_round_trip_and_layout(tmp_path):
    from hsr_utils import mesh
    g = np.random.default_rng(0)
    V, F = 11, 7
    pos = g.standard_normal((V, 3)).astype(np.float32)
    faces = g.integers(0, V, (F, 3)).astype(np.int32)
    rgb = g.integers(0, 256, (V, 3)).astype(np.uint8)
    labels = g.integers(-1, 100000, V).astype(np.int32)
    for with_rgb, with_labels in ((True, True), (True, False), (False, True), (False, False)):
        path = mesh.save_mesh_ply(str(tmp_path / "m.ply"), torch.tensor(pos), faces, rgb if with_rgb else None, torch.tensor(labels) if with_labels else None)
        data = open(path, "rb").read()
        header = (b"ply\nformat binary_little_endian 1.0\nelement vertex 11\nproperty float x\nproperty float y\nproperty float z\n"
                  + (b"property uchar red\nproperty uchar green\nproperty uchar blue\n" if with_rgb else b"")
                  + (b"property int label\n" if with_labels else b"")
                  + b"element face 7\nproperty list uchar int vertex_indices\nend_header\n")
        assert data.startswith(header)
        stride = 12 + 3 * with_rgb + 4 * with_labels
        assert len(data) == len(header) + V * stride + F * 13
        body = data[len(header):]
        for v in (0, V - 1):      # the byte layout of a vertex and of a face, by hand
            rec = body[v * stride:(v + 1) * stride]
            assert rec[:12] == pos[v].astype("<f4").tobytes()
            assert not with_rgb or rec[12:15] == rgb[v].tobytes()
            assert not with_labels or rec[stride - 4:] == labels[v].astype("<i4").tobytes()
        for f in (0, F - 1):
            rec = body[V * stride + 13 * f:V * stride + 13 * (f + 1)]
            assert rec[:1] == b"\x03" and rec[1:] == faces[f].astype("<i4").tobytes()
        got = mesh.load_mesh_ply(path)
        assert np.array_equal(got[0].view(np.uint32), pos.view(np.uint32)) and got[1].dtype == np.int32 and np.array_equal(got[1], faces)
        assert (np.array_equal(got[2], rgb) and got[2].dtype == np.uint8) if with_rgb else got[2] is None
        assert (np.array_equal(got[3], labels) and got[3].dtype == np.int32) if with_labels else got[3] is None
    # an empty mesh is a file too
    path = mesh.save_mesh_ply(str(tmp_path / "e.ply"), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint8))
    got = mesh.load_mesh_ply(path)
    assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and got[2].shape == (0, 3) and got[3] is None
    with pytest.raises(RuntimeError, match="a face index is outside 0..10"):
        mesh.save_mesh_ply(str(tmp_path / "bad.ply"), pos, np.array([[0, 1, 11]], np.int32))
    with pytest.raises(RuntimeError, match=r"rgb must be uint8 \[V,3\]"):
        mesh.save_mesh_ply(str(tmp_path / "bad.ply"), pos, faces, rgb.astype(np.float32))


def test_mesh_bounds_and_its_refusal():
    from hsr_utils import mesh
    means = torch.tensor([[0.0, 0.0, 0.0], [1.0, 2.0, 0.5], [-1.0, 0.25, 3.0], [float("nan"), 50.0, 50.0], [float("inf"), 0.0, 0.0]])
    origin, dims = mesh.mesh_bounds({"means3D": means}, 0.5, 0.25)
    assert origin == (-1.5, -0.5, -0.5) and dims == (13, 13, 17)      # (2, 2, 3) + 1 of padding, every 0.25, plus the far end
    far = np.array(origin) + 0.25 * (np.array(dims) - 1)
    assert (far >= np.array([1.0, 2.0, 3.0]) + 0.5).all()
    assert mesh.mesh_bounds({"means3D": means.numpy()}, 0.0, 1.0) == ((-1.0, 0.0, 0.0), (3, 3, 4))
    with pytest.raises(ValueError, match=r"13 x 13 x 17 = 2873 points, more than max_voxels = 2872; a voxel size of") as e:
        mesh.mesh_bounds({"means3D": means}, 0.5, 0.25, max_voxels=2872)
    fit = float(str(e.value).split("a voxel size of ")[-1].split(" fits")[0])
    assert 0.25 < fit < 0.3
    _o, fitted = mesh.mesh_bounds({"means3D": means}, 0.5, fit, max_voxels=2872)      # the size the message names does fit
    assert int(np.prod(fitted)) <= 2872
    assert mesh.mesh_bounds({"means3D": means}, 0.5, 0.25, max_voxels=2873)[1] == (13, 13, 17)
    with pytest.raises(ValueError, match="max_voxels = 268435456"):      # the default: 2^28
        mesh.mesh_bounds({"means3D": means * 100}, 0.5, 0.01)
    with pytest.raises(ValueError, match="no finite means3D"):
        mesh.mesh_bounds({"means3D": means[3:]}, 0.5, 0.25)
    for bad in (dict(pad=-1.0, voxel_size=0.1), dict(pad=0.1, voxel_size=0.0), dict(pad=0.1, voxel_size=float("nan"))):
        with pytest.raises(ValueError, match="voxel_size must be finite and positive"):
            mesh.mesh_bounds({"means3D": means}, **bad)


def test_host_argument_errors(tmp_path):
    from hsr_utils import mesh, slam
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.TsdfVolume((0, 0, 0), (4, 4, 4), 0.1, device="cpu")
    for dims in ((0, 4, 4), (4, -1, 4), (2048, 1024, 1024)):
        with pytest.raises(ValueError, match="at least 1 a side and X\\*Y\\*Z <= 2\\^31-1"):
            mesh.TsdfVolume((0, 0, 0), dims, 0.1)
    for kw in (dict(voxel_size=0.0), dict(voxel_size=0.1, trunc=-1.0), dict(voxel_size=0.1, max_weight=float("inf"))):
        with pytest.raises(ValueError, match="must be finite and positive"):
            mesh.TsdfVolume((0, 0, 0), (4, 4, 4), **kw)
    params = {"means3D": torch.rand(5, 3), "cam_unnorm_rots": torch.rand(1, 4, 3), "cam_trans": torch.rand(1, 3, 3)}
    with pytest.raises(ValueError, match="every must be >= 1"):
        mesh.mesh_run(params, str(tmp_path / "m.ply"), voxel_size=0.1, every=0)
    with pytest.raises(ValueError, match="label_mode must be one of flat, tree, leaf"):
        mesh.mesh_run(params, str(tmp_path / "m.ply"), voxel_size=0.1, label_mode="argmax")
    with pytest.raises(RuntimeError, match=r"semantic=True needs params\['semantic'\]"):
        mesh.mesh_run(params, str(tmp_path / "m.ply"), voxel_size=0.1, semantic=True)
    assert not os.path.exists(str(tmp_path / "m.ply"))
    session = slam.SlamSession.__new__(slam.SlamSession)
    session.params = None
    with pytest.raises(RuntimeError, match="export_mesh before the first frame"):
        session.export_mesh(str(tmp_path / "s.ply"), voxel_size=0.1)
