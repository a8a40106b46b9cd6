"""CPU suite for the scoring of a run's mesh (include/eval/hsr_mesh_eval.h, hsr_utils.mesh_eval): the header through the helpers of
tests/test_abi.py (its prototypes, that the library exports them and that _abi.EVAL_HEADERS binds them with the header's types); every
refusal of the header with dummy pointers; the lazy names; the numpy restatement (tests/mesh_eval_ref.py) against what it must be — and
its grid search against brute force on every nearest-neighbour fixture, which is the proof of the stopping rule; the host errors of
hsr_utils.mesh_eval.  Nothing here launches: there is no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_eval_ref as R
import test_abi

HEADER = "eval/hsr_mesh_eval.h"
NAMES = ["hsr_mesh_areas", "hsr_mesh_sample", "hsr_mesh_seen", "hsr_nn_cells", "hsr_nn_pack", "hsr_nn_query"]
FP, VP, IP, LP, DP = ("pointer", "float"), ("pointer", "void"), ("pointer", "int"), ("pointer", "int64_t"), ("pointer", "double")
NAN, INF = float("nan"), float("inf")


def test_mesh_eval_abi_exported_and_bound():
    from diff_gaussian_rasterization import _abi
    protos = test_abi._prototypes([HEADER])
    assert list(_abi.EVAL_HEADERS) == [HEADER] and HEADER not in _abi.HEADERS and HEADER not in test_abi.ALL_HEADERS
    assert [s[0] for s in _abi.EVAL_HEADERS[HEADER]] == list(protos) == NAMES
    assert test_abi.check_header(HEADER) == NAMES      # exported, and bound with the header's type classes
    for name, restype, argtypes in _abi.EVAL_HEADERS[HEADER]:      # _load() bound this table as it binds HEADERS
        fn = getattr(_abi.lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert not set(NAMES) & {s[0] for table in _abi.HEADERS.values() for s in table}
    assert protos["hsr_mesh_areas"][1:] == ("int", ["int", "int", FP, IP, FP, VP])
    assert protos["hsr_mesh_sample"][1:] == ("int", ["int", "int", "int", "size_t", FP, IP, DP, IP, FP, IP, IP, VP])
    assert protos["hsr_mesh_seen"][1:] == ("int", ["int", FP, "int", "int"] + ["float"] * 4 + [FP, FP, "float", ("pointer", "uint8_t"), VP])
    assert protos["hsr_nn_cells"][1:] == ("int", ["int"] * 3 + ["float"] * 4 + ["int", FP, IP, VP])
    assert protos["hsr_nn_pack"][1:] == ("int", ["int", FP, LP, VP, VP])
    assert protos["hsr_nn_query"][1:] == ("int", ["int"] * 3 + ["float"] * 4 + ["int", IP, VP, "int", FP, FP, IP, VP])
    assert _abi.lib.hsr_mesh_seen.argtypes[8] is _abi.fp      # w2c is the one HOST pointer: a ctypes array goes in by address
    from hsr_utils import mesh_eval
    source = test_abi._source(HEADER)
    for name, value in (("HSR_MESH_MAX_IMAGE_SIDE", mesh_eval.MAX_IMAGE_SIDE), ("HSR_NN_MAX_SIDE", mesh_eval.MAX_SIDE),
                        ("HSR_NN_MAX_CELLS", mesh_eval.MAX_CELLS)):
        assert "#define %s %d\n" % (name, value) in source
    assert (mesh_eval.MAX_SIDE, mesh_eval.MAX_CELLS) == (1024, 2 ** 24)


def test_names_are_reached_lazily_from_the_package():
    import hsr_utils
    from hsr_utils import mesh, mesh_eval
    assert tuple(hsr_utils._MESH_EVAL) == tuple(mesh_eval.__all__)
    for name in hsr_utils._MESH_EVAL:
        assert getattr(hsr_utils, name) is getattr(mesh_eval, name), name
    assert set(hsr_utils._MESH) == set(mesh.__all__) and not set(hsr_utils._MESH) & set(hsr_utils._MESH_EVAL)
    assert callable(hsr_utils.SlamSession.evaluate_mesh)


# ---- refusals: dummy non-device pointers that are never followed ---------------------------------------------------------------------------
W2C = (C.c_float * 16)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1)
D = [4096 * (n + 1) for n in range(8)]      # 16-byte aligned


def areas_call(lib, V=4, F=2, vertices=D[0], faces=D[1], out_area=D[2]):
    return lib.hsr_mesh_areas(V, F, vertices, faces, out_area, None)


def sample_call(lib, V=4, F=2, S=5, vertices=D[0], faces=D[1], cum=D[2], vertex_labels=D[3], out_points=D[4], out_face=D[5], out_label=D[6]):
    return lib.hsr_mesh_sample(V, F, S, 7, vertices, faces, cum, vertex_labels, out_points, out_face, out_label, None)


def seen_call(lib, V=4, vertices=D[0], H=6, W=8, w2c=W2C, depth=D[1], eps=0.05, seen=D[2]):
    return lib.hsr_mesh_seen(V, vertices, H, W, 8.0, 8.0, 3.5, 2.5, w2c, depth, eps, seen, None)


def cells_call(lib, X=4, Y=3, Z=2, ox=0.0, c=0.1, M=5, points=D[0], out_cell=D[1]):
    return lib.hsr_nn_cells(X, Y, Z, ox, 0.0, 0.0, c, M, points, out_cell, None)


def pack_call(lib, M=5, points=D[0], order=D[1], out_packed=D[2]):
    return lib.hsr_nn_pack(M, points, order, out_packed, None)


def query_call(lib, X=4, Y=3, Z=2, ox=0.0, c=0.1, M=5, cell_start=D[0], packed=D[1], N=3, queries=D[2], out_d2=D[3], out_index=D[4]):
    return lib.hsr_nn_query(X, Y, Z, ox, 0.0, 0.0, c, M, cell_start, packed, N, queries, out_d2, out_index, None)


GRIDS = ([(dict(X=0), b"invalid grid X=0"), (dict(Y=-1), b"invalid grid"), (dict(Z=0), b"invalid grid X=4 Y=3 Z=0"),
          (dict(X=1025), b"every side 1..1024"), (dict(Z=1025), b"invalid grid"), (dict(X=512, Y=512, Z=65), b"X*Y*Z <= 2^24"),
          (dict(X=1024, Y=1024, Z=1024), b"invalid grid")]
         + [(dict(c=v), b"must be finite and positive") for v in (0.0, -0.1, NAN, INF, -INF)]
         + [(dict(ox=v), b"the origin finite") for v in (NAN, INF)])
REFUSALS = (
    [(areas_call, b"mesh_areas: ", o, b"invalid sizes") for o in (dict(V=0), dict(V=-2), dict(F=-1))]
    + [(areas_call, b"mesh_areas: ", {n: None}, b"are required with F > 0") for n in ("vertices", "faces", "out_area")]
    + [(sample_call, b"mesh_sample: ", o, b"invalid sizes") for o in (dict(V=0), dict(F=0), dict(F=-1), dict(S=-1))]
    + [(sample_call, b"mesh_sample: ", {n: None}, b"are required with S > 0") for n in ("vertices", "faces", "cum", "out_points", "out_face")]
    + [(sample_call, b"mesh_sample: ", {n: None}, b"come together") for n in ("vertex_labels", "out_label")]
    + [(seen_call, b"mesh_seen: ", dict(V=-1), b"invalid size V=-1")]
    + [(seen_call, b"mesh_seen: ", o, b"invalid image size") for o in (dict(H=0), dict(W=0), dict(H=16385), dict(W=16385), dict(H=-4))]
    + [(seen_call, b"mesh_seen: ", dict(eps=v), b"eps must be finite and not negative") for v in (-0.01, NAN, INF)]
    + [(seen_call, b"mesh_seen: ", {n: None}, b"is required") for n in ("w2c", "vertices", "seen")]
    + [(cells_call, b"nn_cells: ", o, m) for o, m in GRIDS]
    + [(cells_call, b"nn_cells: ", o, b"must be >= 0") for o in (dict(M=-1), dict(points=None), dict(out_cell=None))]
    + [(pack_call, b"nn_pack: ", o, b"must be >= 0") for o in (dict(M=-1), dict(points=None), dict(order=None), dict(out_packed=None))]
    + [(pack_call, b"nn_pack: ", dict(out_packed=D[2] + 4), b"16-byte aligned")]
    + [(query_call, b"nn_query: ", o, m) for o, m in GRIDS]
    + [(query_call, b"nn_query: ", o, b"invalid sizes") for o in (dict(N=-1), dict(M=0), dict(M=-3))]
    + [(query_call, b"nn_query: ", {n: None}, b"are required with N > 0") for n in ("cell_start", "packed", "queries", "out_d2", "out_index")]
    + [(query_call, b"nn_query: ", dict(packed=D[1] + 8), b"16-byte aligned")]
)


@pytest.mark.parametrize("call,prefix,overrides,message", REFUSALS, ids=["%d" % i for i in range(len(REFUSALS))])
def test_entry_points_refuse_before_any_device_work(call, prefix, overrides, message):
    from diff_gaussian_rasterization import _abi
    rc = call(_abi.lib, **overrides)
    err = _abi.lib.hsr_last_error()
    assert rc == -1 and err.startswith(prefix) and message in err, (overrides, rc, err)


def test_nothing_to_do_launches_nothing():
    """a count of 0 returns before any device work, whatever the pointers are"""
    from diff_gaussian_rasterization import _abi
    lib = _abi.lib
    assert areas_call(lib, F=0, vertices=None, faces=None, out_area=None) == 0
    assert sample_call(lib, S=0, vertices=None, faces=None, cum=None, out_points=None, out_face=None) == 0
    assert seen_call(lib, V=0, vertices=None, seen=None) == 0
    assert cells_call(lib, M=0, points=None, out_cell=None) == 0
    assert pack_call(lib, M=0, points=None, order=None, out_packed=None) == 0
    assert query_call(lib, N=0, cell_start=None, packed=None, queries=None, out_d2=None, out_index=None) == 0


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def test_areas_and_sampler_restatement():
    area = R.areas(R.TRI_VERTICES, R.TRI_FACES)
    assert area.dtype == np.float32 and area.tolist() == [1.0, 0.0, 3.0]
    bad = np.concatenate([R.TRI_FACES, [[0, 1, 7]], [[-1, 1, 2]]]).astype(np.int32)
    assert R.areas(R.TRI_VERTICES, bad).tolist() == [1.0, 0.0, 3.0, 0.0, 0.0]
    assert R.splitmix(0, 1) == 0xE220A8397B1DCDAF      # the first output of splitmix64 seeded with 0
    cum = np.cumsum(area.astype(np.float64))
    counts = []
    for seed in range(4):
        points, face, labels = R.sample(R.TRI_VERTICES, R.TRI_FACES, cum, 4096, seed, R.TRI_LABELS)
        assert not (face == 1).any() and set(face.tolist()) == {0, 2}
        counts.append(int((face == 0).sum()))
        assert 1024 - 111 <= counts[-1] <= 1024 + 111      # 4 binomial standard deviations of sqrt(4096 * 1/4 * 3/4) = 27.7
        assert (points[:, 2] == 0).all() and (points[:, :2] >= 0).all() and (points[:, 0] <= 3).all() and (points[:, 1] <= 2).all()
        in_first = points[:, 0] + points[:, 1] / 2 <= 1 + 1e-6      # the triangle (0,0), (1,0), (0,2)
        assert np.array_equal(in_first, face == 0)
        # the label is the nearest corner's, so the corner at the origin labels the samples nearest to it
        assert set(labels[face == 0].tolist()) <= {10, 11, 12} and set(labels[face == 2].tolist()) <= {14, 15, 16}
    assert counts == [1013, 1066, 1040, 1014]
    again = R.sample(R.TRI_VERTICES, R.TRI_FACES, cum, 64, 3, R.TRI_LABELS)
    assert np.array_equal(again[0], points[:64]) and np.array_equal(again[1], face[:64])      # counter-based: sample s does not depend on S


def test_cells_restatement_clamps_and_sends_nan_to_zero():
    pts = np.array([[0.05, 0.05, 0.05], [0.35, 0.25, 0.15], [-5, 0.05, 9], [NAN, 0.25, 0.05], [INF, -INF, 0.05], [0.4, 0.3, 0.2]], np.float32)
    assert R.cells(pts, (0.0, 0.0, 0.0), 0.1, (4, 3, 2)).tolist() == [0, (1 * 3 + 2) * 4 + 3, (1 * 3 + 0) * 4 + 0, (0 * 3 + 2) * 4 + 0, 3, 23]


def test_seen_restatement():
    k = np.array([[8.0, 0, 3.5], [0, 8.0, 2.5], [0, 0, 1]])
    H, W = 6, 8
    # u = 8 x / z + 3.5 and floor(u + 0.5) in 0..7: at z = 1, x = -0.5 gives u = -0.5 -> 0 (in) and just below gives -1 (out); x = 0.5
    # gives u = 7.5 -> 8 (out) and just below gives 7 (in); v = 8 y + 2.5 in -0.5 <= v < 5.5 likewise
    pts = np.array([[0, 0, 1], [0, 0, -1], [0, 0, 0], [-0.5, 0, 1], [-0.5001, 0, 1], [0.4999, 0, 1], [0.5, 0, 1], [0, -0.375, 1], [0, -0.3751, 1],
                    [0, 0.3749, 1], [0, 0.375, 1]], np.float32)
    assert R.seen(pts, np.eye(4), k, H, W).tolist() == [1, 0, 0, 1, 0, 1, 0, 1, 0, 1, 0]
    depth = np.full((H, W), 0.9, np.float32)
    assert R.seen(pts[:1], np.eye(4), k, H, W, depth, eps=0.05).tolist() == [0] and R.seen(pts[:1], np.eye(4), k, H, W, depth, eps=0.11).tolist() == [1]
    for bad in (0.0, NAN, INF, -1.0):
        depth[3, 4] = bad      # the pixel of (0, 0, 1): column floor(3.5 + 0.5) = 4, row floor(2.5 + 0.5) = 3
        assert R.seen(pts[:1], np.eye(4), k, H, W, depth, eps=10.0).tolist() == [0]
    kept = R.seen(pts, np.eye(4), k, H, W, out=np.array([0, 1] + [0] * 9, np.uint8))
    assert kept.tolist() == [1, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0]      # nothing is cleared


FIXTURES = R.nn_fixtures()


@pytest.mark.parametrize("name", list(FIXTURES))
def test_grid_search_equals_brute_force(name):
    """the stopping rule of hsr_nn_query, restated as a loop, gives brute force's values AND indices"""
    queries, targets, cell = FIXTURES[name]
    origin, c, dims = R.grid_of(targets, cell)
    assert max(dims) <= 1024 and np.prod(dims) <= 2 ** 24
    want_d2, want_index = R.brute_nn(queries, targets)
    rings = []
    got_d2, got_index = R.grid_nn(queries, targets, origin, c, dims, stats=rings)
    assert np.array_equal(got_d2.view(np.uint32), want_d2.view(np.uint32)) and np.array_equal(got_index, want_index)
    if name == "flat_Z1":
        assert dims[2] == 1
    if name == "cluster_far":
        assert max(rings) >= 17      # queries there walk many empty rings
    if name == "lattice_twice":      # exact ties: half the lattice points stored twice are reached by the smaller index only
        assert (want_index < 125).all() and (want_d2 == 0).sum() == 125
    if name == "nan_query":
        bad = np.isnan(queries).any(axis=1)
        assert bad.sum() == 3 and (want_index[bad] == -1).all() and np.isinf(want_d2[bad]).all() and (want_index[~bad] >= 0).all()
    if name == "nan_target":
        assert not np.isin(want_index, [0, 5, 17]).any()
    if name == "hand_first_hit":
        assert want_index.tolist() == [1] and rings == [1]      # the neighbour across the face wins; "stop at the first hit" would give 0
        own = R.cells(queries, origin, c, dims)[0]
        assert R.cells(targets, origin, c, dims).tolist()[:2] == [own, own - 1]


def test_a_first_hit_rule_would_fail_the_hand_case():
    queries, targets, cell = FIXTURES["hand_first_hit"]
    d2 = R.d2_matrix(queries, targets)[0]
    assert abs(np.sqrt(d2[0]) - 0.9 * cell) < 1e-6 and abs(np.sqrt(d2[1]) - 0.1 * cell) < 1e-6


def test_metrics_restatement():
    m = R.metrics(np.array([0.0, 0.0025, 0.01]), np.array([0.0009, 0.0009]), 0.05)
    assert abs(m["accuracy"] - 0.05) < 1e-15 and abs(m["completion"] - 0.03) < 1e-15 and m["completion_ratio"] == 1.0
    assert abs(m["accuracy_ratio"] - 2 / 3) < 1e-15 and abs(m["f_score"] - 0.8) < 1e-15 and abs(m["chamfer"] - 0.04) < 1e-15
    assert R.metrics(np.array([1.0]), np.array([1.0]), 0.05)["f_score"] == 0.0
    lab = R.metrics(np.zeros(2), np.zeros(5), 0.05, gt_labels=np.array([0, 0, 1, -1, 1]), rec_labels=np.array([0, 1, 5]),
                    nearest=np.array([0, 1, 1, 0, -1]), num_classes=3)
    assert lab["confusion"].tolist() == [[1, 1, 0], [0, 1, 0], [0, 0, 0]]
    assert abs(lab["label_accuracy"] - 2 / 3) < 1e-15 and abs(lab["miou"] - 0.5) < 1e-15      # classes 0 and 1: 1/2 each; class 2 is absent


# ---- the host side -------------------------------------------------------------------------------------------------------------------------
def test_cull_mesh_is_plain_torch():
    from hsr_utils import mesh_eval
    vertices = torch.arange(15, dtype=torch.float32).reshape(5, 3)
    faces = torch.tensor([[0, 1, 2], [1, 2, 3], [2, 3, 4], [4, 2, 1]], dtype=torch.int32)
    labels = torch.tensor([5, 6, 7, 8, 9], dtype=torch.int32)
    seen = torch.tensor([0, 1, 1, 1, 1], dtype=torch.uint8)
    v, f, lab, none = mesh_eval.cull_mesh(vertices, faces, seen, labels, None)
    assert torch.equal(v, vertices[1:]) and f.dtype == torch.int32 and f.tolist() == [[0, 1, 2], [1, 2, 3], [3, 1, 0]]
    assert lab.tolist() == [6, 7, 8, 9] and none is None
    v, f = mesh_eval.cull_mesh(vertices, faces, torch.zeros(5, dtype=torch.bool))
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_host_value_errors(tmp_path):
    from hsr_utils import mesh_eval, slam
    with pytest.raises(ValueError, match="the mesh has no faces"):
        mesh_eval.sample_mesh(torch.zeros(3, 3), torch.zeros((0, 3), dtype=torch.int32), 10)
    with pytest.raises(ValueError, match="no finite point"):
        mesh_eval.NearestGrid(torch.tensor([[NAN, 0.0, 0.0], [0.0, INF, 1.0]]), 0.1)
    with pytest.raises(ValueError, match="no finite point"):
        mesh_eval.NearestGrid(torch.zeros(0, 3), 0.1)
    for cell in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError, match="cell must be finite and positive"):
            mesh_eval.NearestGrid(torch.zeros(4, 3), cell)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh_eval.NearestGrid(torch.zeros(4, 3), 0.1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh_eval.sample_mesh(torch.zeros(3, 3), torch.zeros((1, 3), dtype=torch.int32), 10)
    with pytest.raises(ValueError, match="n_samples must be >= 1"):
        mesh_eval.mesh_metrics((torch.zeros(3, 3), torch.zeros((1, 3))), (torch.zeros(3, 3), torch.zeros((1, 3))), n_samples=0)
    with pytest.raises(ValueError, match="eps must be finite and not negative"):
        mesh_eval.seen_vertices(torch.zeros(3, 3), np.eye(4)[None], np.eye(3), 4, 4, eps=-1.0)
    with pytest.raises(ValueError, match="the image is 4 x 0"):
        mesh_eval.seen_vertices(torch.zeros(3, 3), np.eye(4)[None], np.eye(3), 0, 4)
    session = slam.SlamSession.__new__(slam.SlamSession)
    session.params = None
    with pytest.raises(RuntimeError, match="evaluate_mesh before the first frame"):
        session.evaluate_mesh(str(tmp_path / "gt.ply"), voxel_size=0.1)
