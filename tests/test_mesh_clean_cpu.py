"""CPU suite for the components of a mesh and their removal (include/surface/hsr_mesh_clean.h, hsr_utils.mesh_clean): the numpy
restatement (tests/mesh_clean_ref.py) against a brute-force flood fill and against itself under random face orders; the header through
the helpers of tests/test_abi.py (its prototypes, that the library exports them and that _abi.SURFACE_HEADERS binds them with the header's
types); every refusal of the header with dummy pointers; the scratch size; the lazy names; component_keep's rules on CPU tensors; the host
errors; that mesh_run and what forwards to it carry the three keywords.  Nothing here launches: there is no GPU."""
import inspect

import numpy as np
import pytest
import torch

import mesh_clean_ref as R
import test_abi
import tsdf_ref

HEADER = "surface/hsr_mesh_clean.h"
NAMES = ["hsr_mesh_components", "hsr_mesh_select_scratch_bytes", "hsr_mesh_select"]
VP, IP = ("pointer", "void"), ("pointer", "int")


# ---- the restatement --------------------------------------------------------------------------------------------------------------------------
def random_mesh(rng, V, F, bad=0):
    faces = rng.integers(0, V, (F, 3)).astype(np.int32)
    for _ in range(bad):
        faces[rng.integers(0, F), rng.integers(0, 3)] = rng.choice([-1, V, V + 7, -5])
    return faces


@pytest.mark.parametrize("seed", range(12))
def test_restatement_equals_a_flood_fill_on_random_meshes(seed):
    rng = np.random.default_rng(seed)
    V = int(rng.integers(1, 60))
    F = int(rng.integers(0, max(1, V // 2)))      # sparse: many components and unreferenced vertices
    faces = random_mesh(rng, V, F, bad=seed % 3 if F else 0)
    label, count = R.components(faces, V)
    want_label, want_count = R.flood_fill(faces, V)
    assert label.dtype == count.dtype == np.int32 and label.shape == count.shape == (V,)
    assert np.array_equal(label, want_label) and np.array_equal(count, want_count)
    assert (label <= np.arange(V)).all() and (label[label] == label).all()      # the smallest index, and a label is its own label
    assert count.sum() == R.valid_faces(faces, V).sum() and (count[label != np.arange(V)] == 0).all()
    for _ in range(3):      # the order in which the faces are united does not matter
        again = R.components(faces, V, order=rng.permutation(F))
        assert np.array_equal(again[0], label) and np.array_equal(again[1], count)


def test_restatement_on_the_meshes_of_the_device_suite():
    for numbering in ("ascending", "descending", "permuted"):
        faces, V = R.strip(300, numbering)
        label, count = R.components(faces, V)
        assert (label == 0).all() and count[0] == 300 and count.sum() == 300
    for hub in ("first", "last"):
        faces, V = R.fan(200, hub)
        label, count = R.components(faces, V)
        assert (label == 0).all() and count[0] == 200
    faces, V = R.disjoint(2 * R.BLOCK + 1)
    label, count = R.components(faces, V)
    assert np.array_equal(label, 3 * (np.arange(V) // 3)) and np.array_equal(count, (np.arange(V) % 3 == 0).astype(np.int32))
    faces, V, n = R.patches()
    label, count = R.components(faces, V)
    assert n == 36 and (count > 0).sum() == n and len(set(count[count > 0].tolist())) >= 10      # patches of many sizes
    assert np.array_equal(label, R.flood_fill(faces, V)[0])
    assert (np.bincount(faces.reshape(-1), minlength=V) == 0).sum() > 100      # the cuts left unreferenced vertices behind


def test_restatement_of_select():
    faces = np.array([[4, 5, 6], [0, 1, 2], [9, 2, 0], [7, 7, 8], [0, 1, 10], [-1, 1, 2]], np.int32)      # V = 10: two invalid faces
    V = 10
    label, count = R.components(faces, V)
    assert label.tolist() == [0, 0, 0, 3, 4, 4, 4, 7, 7, 0] and count.tolist() == [2, 0, 0, 0, 1, 0, 0, 1, 0, 0]
    out, source = R.select(faces, V, label, R.keep(count))      # everything with a face: vertex 3 goes, the invalid faces go
    assert source.tolist() == [0, 1, 2, 4, 5, 6, 7, 8, 9] and out.tolist() == [[3, 4, 5], [0, 1, 2], [8, 2, 0], [6, 6, 7]]
    out, source = R.select(faces, V, label, R.keep(count, min_faces=2))
    assert source.tolist() == [0, 1, 2, 9] and out.tolist() == [[0, 1, 2], [3, 2, 0]]
    out, source = R.select(faces, V, label, np.zeros(V, np.uint8))
    assert out.shape == (0, 3) and source.shape == (0,) and out.dtype == source.dtype == np.int32
    out, source = R.select(faces, V, np.full(V, V, np.int32), np.ones(V, np.uint8))      # a label outside 0..V-1 drops the face
    assert out.shape == (0, 3) and source.shape == (0,)
    vertices = np.arange(30, dtype=np.float32).reshape(10, 3)
    v, f, s = R.clean(vertices, faces, largest=True)
    assert s.tolist() == [0, 1, 2, 9] and np.array_equal(v, vertices[s]) and f.tolist() == [[0, 1, 2], [3, 2, 0]]


# ---- the real extraction of tests/test_gpu_mesh_clean.py ---------------------------------------------------------------------------------------
DIMS, H, TRUNC = (24, 16, 14), 0.05, 0.2
BIG, SMALL = ((0.40, 0.40, 0.35), 0.22), ((0.98, 0.40, 0.35), 0.07)


def two_spheres():
    """(both spheres, the large one alone) as tsdf_ref volumes with colour and labels: the pointwise minimum of the two distance fields"""
    big = tsdf_ref.sphere_volume(DIMS, H, BIG[0], BIG[1], TRUNC, color=True, labels=True)
    small = tsdf_ref.sphere_volume(DIMS, H, SMALL[0], SMALL[1], TRUNC, color=True, labels=True)
    both = big.copy()
    both.tsdf = np.minimum(big.tsdf, small.tsdf)
    for vol in (big, both):
        vol.color[:] = np.linspace(0, 1, vol.N, dtype=np.float32)
        vol.cweight[:] = 1
        vol.label[:] = np.arange(vol.N, dtype=np.int32)
    return both, big


def test_two_spheres_clean_to_the_large_one_bit_for_bit():
    """what the device test asks of clean_mesh, by the restatements alone: 2 416 faces in two closed components of 2 232 and 184, and
    without the small one the extraction of the large sphere alone"""
    both, big = two_spheres()
    pos, faces, rgb, labels, _keys = tsdf_ref.extract(both)
    want_pos, want_faces, want_rgb, want_labels, _keys = tsdf_ref.extract(big)
    label, count = R.components(faces, len(pos))
    assert len(faces) == 2416 and sorted(count[count > 0].tolist()) == [184, 2232] and len(want_faces) == 2232
    for root in np.flatnonzero(count):
        assert tsdf_ref.topology(faces[label[faces[:, 0]] == root]) == (True, 2)      # closed, a sphere
    got_pos, got_faces, src = R.clean(pos, faces, min_faces=185)
    assert np.array_equal(got_faces, want_faces) and tsdf_ref.same_floats(got_pos, want_pos)
    assert np.array_equal(rgb[src], want_rgb) and np.array_equal(labels[src], want_labels) and len(np.unique(want_labels)) > 100


# ---- the header ------------------------------------------------------------------------------------------------------------------------------
def test_mesh_clean_abi_exported_and_bound():
    from diff_gaussian_rasterization import _abi
    protos = test_abi._prototypes([HEADER])
    assert list(_abi.SURFACE_HEADERS) == [HEADER] and HEADER not in test_abi.ALL_HEADERS
    others = (_abi.HEADERS, _abi.EVAL_HEADERS, _abi.RECON_HEADERS, _abi.SENSOR_HEADERS)
    assert all(HEADER not in table for table in others)
    assert [s[0] for s in _abi.SURFACE_HEADERS[HEADER]] == list(protos) == NAMES      # the header's names in the header's order
    assert test_abi.check_header(HEADER) == NAMES      # exported, and bound with the header's type classes
    for name, restype, argtypes in _abi.SURFACE_HEADERS[HEADER]:      # _load() bound this table as it binds the other four
        fn = getattr(_abi.lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    bound = [s[0] for tables in others + (_abi.SURFACE_HEADERS,) for table in tables.values() for s in table]
    assert sorted(bound) == sorted(set(bound))      # no name twice across the five tables
    assert protos["hsr_mesh_components"][1:] == ("int", ["int", "int", IP, IP, IP, VP])
    assert protos["hsr_mesh_select_scratch_bytes"][1:] == ("size_t", ["int", "int"])
    assert protos["hsr_mesh_select"][1:] == ("int", ["int", "int", IP, IP, ("pointer", "uint8_t"), IP, IP, ("pointer", "int64_t"), VP, "size_t", VP])
    from hsr_utils import mesh_clean
    source = test_abi._source(HEADER)
    assert "#define HSR_MESH_CLEAN_BLOCK %d\n" % mesh_clean.BLOCK in source and mesh_clean.BLOCK == R.BLOCK


def test_names_are_reached_lazily_from_the_package():
    import hsr_utils
    from hsr_utils import mesh, mesh_clean, mesh_eval, slam
    assert tuple(hsr_utils._MESH_CLEAN) == tuple(mesh_clean.__all__)
    for name in hsr_utils._MESH_CLEAN:
        assert getattr(hsr_utils, name) is getattr(mesh_clean, name), name
    assert not set(hsr_utils._MESH_CLEAN) & (set(hsr_utils._MESH_DEPTH) | set(hsr_utils._MESH_EVAL) | set(hsr_utils._MESH))
    # every new keyword of mesh_run defaults to "off", and what calls mesh_run forwards keywords it does not know
    keywords = inspect.signature(mesh.mesh_run).parameters
    assert [keywords[n].default for n in ("min_component_faces", "min_component_ratio", "largest_component")] == [0, 0.0, False]
    for fn in (mesh_eval.evaluate_mesh_run, slam.SlamSession.export_mesh, slam.SlamSession.evaluate_mesh):
        assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in inspect.signature(fn).parameters.values()), fn


# ---- refusals: dummy non-device pointers that are never followed ---------------------------------------------------------------------------
D = [4096 * (n + 1) for n in range(8)]      # 16-byte aligned


def components_call(lib, V=4, F=2, faces=D[0], out_label=D[1], out_face_count=D[2]):
    return lib.hsr_mesh_components(V, F, faces, out_label, out_face_count, None)


def select_call(lib, V=4, F=2, faces=D[0], label=D[1], keep=D[2], out_faces=D[3], out_source=D[4], out_counts=D[5], scratch=D[6], scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = lib.hsr_mesh_select_scratch_bytes(max(V, 0), max(F, 0))
    return lib.hsr_mesh_select(V, F, faces, label, keep, out_faces, out_source, out_counts, scratch, scratch_bytes, None)


COMPONENT_REFUSALS = (
    [(o, b"invalid sizes") for o in (dict(V=-1), dict(F=-1), dict(V=-3, F=-3))]
    + [(dict(faces=None), b"faces is required with F > 0")]
    + [({n: None}, b"are required with V > 0") for n in ("out_label", "out_face_count")]
)
SELECT_REFUSALS = (
    [(o, b"invalid sizes") for o in (dict(V=-1), dict(F=-1))]
    + [({n: None}, b"are required with F > 0") for n in ("faces", "out_faces")]
    + [({n: None}, b"are required with V > 0") for n in ("label", "keep", "out_source")]
    + [(dict(out_counts=None), b"out_counts is required")]
    + [(dict(scratch=None), b"the scratch must hold"), (dict(scratch_bytes=0), b"the scratch must hold"),
       (dict(scratch_bytes=16 + 16 + 16 + 16 - 1), b"the scratch must hold")]
    + [(dict(scratch=D[6] + 8), b"16-byte aligned"), (dict(scratch=D[6] + 4), b"16-byte aligned")]
)


@pytest.mark.parametrize("overrides,message", COMPONENT_REFUSALS, ids=["%d" % i for i in range(len(COMPONENT_REFUSALS))])
def test_components_refuses_before_any_device_work(overrides, message):
    from diff_gaussian_rasterization import _abi
    rc = components_call(_abi.lib, **overrides)
    err = _abi.lib.hsr_last_error()
    assert rc == -1 and err.startswith(b"mesh_components: ") and message in err, (overrides, rc, err)


@pytest.mark.parametrize("overrides,message", SELECT_REFUSALS, ids=["%d" % i for i in range(len(SELECT_REFUSALS))])
def test_select_refuses_before_any_device_work(overrides, message):
    from diff_gaussian_rasterization import _abi
    rc = select_call(_abi.lib, **overrides)
    err = _abi.lib.hsr_last_error()
    assert rc == -1 and err.startswith(b"mesh_select: ") and message in err, (overrides, rc, err)


def test_components_of_no_vertices_launches_nothing():
    from diff_gaussian_rasterization import _abi
    assert _abi.lib.hsr_mesh_components(0, 0, None, None, None, None) == 0      # there is no device here: a launch would fail
    assert _abi.lib.hsr_mesh_components(0, 3, D[0], None, None, None) == 0


def test_scratch_bytes_is_monotone_and_positive():
    from diff_gaussian_rasterization import _abi
    size = _abi.lib.hsr_mesh_select_scratch_bytes
    assert size(0, 0) == 16 and size(-1, 0) == 0 and size(0, -1) == 0
    assert size(4, 2) == 16 + 16 + 16 + 16      # four new indices, one count of each list rounded up to 16 bytes, and 16 more
    sizes = (0, 1, 3, 4, 5, 255, 256, 257, 1024, 1025, 10 ** 6, 2 ** 31 - 1)
    by_vertices = [size(V, 1000) for V in sizes]
    by_faces = [size(1000, F) for F in sizes]
    assert by_vertices == sorted(by_vertices) and by_faces == sorted(by_faces) and all(b % 16 == 0 for b in by_vertices + by_faces)
    assert by_vertices[0] < by_vertices[4] < by_vertices[-1] and by_faces[0] < by_faces[-2] < by_faces[-1]
    assert by_vertices[-1] >= 4 * (2 ** 31 - 1)      # past 2^32: the size is a size_t
    assert size(10 ** 6, 2 * 10 ** 6) >= 4 * 10 ** 6 + 4 * (2 * 10 ** 6 // 256) + 4 * (10 ** 6 // 256)


# ---- component_keep ----------------------------------------------------------------------------------------------------------------------------
def test_component_keep_rules():
    from hsr_utils import mesh_clean
    count = torch.tensor([0, 7, 0, 7, 3, 1, 0, 2], dtype=torch.int32)

    def got(**kw):
        out = mesh_clean.component_keep(count, **kw)
        assert out.dtype == torch.uint8 and out.shape == count.shape and np.array_equal(out.numpy(), R.keep(count.numpy(), **kw)), kw
        return out.tolist()

    assert got() == [0, 1, 0, 1, 1, 1, 0, 1]      # everything with a face: an index that is no label is never kept
    assert got(min_faces=1) == got() and got(min_ratio=0.0) == got()
    assert got(min_faces=3) == [0, 1, 0, 1, 1, 0, 0, 0] and got(min_faces=4) == [0, 1, 0, 1, 0, 0, 0, 0] and got(min_faces=8) == [0] * 8
    assert got(min_ratio=1.0) == [0, 1, 0, 1, 0, 0, 0, 0]      # the largest ones, all of them
    assert got(min_ratio=0.25) == [0, 1, 0, 1, 1, 0, 0, 1]     # ceil(1.75) = 2
    assert got(min_ratio=2 / 7) == [0, 1, 0, 1, 1, 0, 0, 1] and got(min_ratio=0.3) == [0, 1, 0, 1, 1, 0, 0, 0]      # ceil(2.1) = 3
    assert got(min_ratio=0.2, min_faces=3) == got(min_faces=3)      # the larger of the two thresholds
    assert got(largest=True) == [0, 1, 0, 0, 0, 0, 0, 0]       # a tie: the smallest label
    assert got(largest=True, min_faces=8) == [0] * 8           # the thresholds still apply
    zero = torch.zeros(5, dtype=torch.int32)
    assert mesh_clean.component_keep(zero).tolist() == [0] * 5 and mesh_clean.component_keep(zero, largest=True).tolist() == [0] * 5
    assert mesh_clean.component_keep(zero, min_ratio=1.0).tolist() == [0] * 5      # no face at all: nothing to keep
    empty = mesh_clean.component_keep(torch.zeros(0, dtype=torch.int32), largest=True)
    assert empty.dtype == torch.uint8 and empty.shape == (0,) and R.keep(np.zeros(0, np.int32)).shape == (0,)
    big = torch.tensor([2 ** 31 - 1, 2 ** 30], dtype=torch.int32)      # float64 holds every count: no rounding at the top
    assert mesh_clean.component_keep(big, min_ratio=1.0).tolist() == [1, 0] and mesh_clean.component_keep(big, min_ratio=0.5).tolist() == [1, 1]
    for bad in (dict(min_faces=-1), dict(min_ratio=-0.1), dict(min_ratio=1.5), dict(min_ratio=float("nan")), dict(min_ratio=float("inf"))):
        with pytest.raises(ValueError, match="min_faces must be >= 0" if "min_faces" in bad else r"min_ratio must be in \[0, 1\]"):
            mesh_clean.component_keep(count, **bad)


# ---- the host side -------------------------------------------------------------------------------------------------------------------------
def test_host_errors():
    from hsr_utils import mesh_clean
    v, f = torch.zeros(3, 3), torch.zeros((1, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="faces must be a tensor on a HIP device; there is no CPU path"):
        mesh_clean.mesh_components(f, 3)
    with pytest.raises(RuntimeError, match="faces must be a tensor on a HIP device; there is no CPU path"):
        mesh_clean.mesh_components(f.numpy(), 3)
    with pytest.raises(RuntimeError, match="vertices must be a tensor on a HIP device; there is no CPU path"):
        mesh_clean.clean_mesh(v, f)
    with pytest.raises(ValueError, match="the number of vertices must be"):
        mesh_clean.mesh_components(f, -1)
