"""GPU suite for the components of a mesh and their removal (include/surface/hsr_mesh_clean.h, hsr_utils.mesh_clean): hsr_mesh_components
and hsr_mesh_select against the numpy restatement (tests/mesh_clean_ref.py) on the smallest meshes at which each mechanism can fail;
clean_mesh on a real extraction; mesh_run with and without the new keywords.  A poisoned tail follows every output.

Derivable, not measured: every output is an integer and a unique function of the input, so the expectation is EQUALITY with the
restatement, and of two runs with each other; no tolerance applies.  No walk may give up: no count is negative anywhere."""
import random

import numpy as np
import pytest
import torch

import mesh_clean_ref as R
import test_gpu_slam_session as TS
import test_mesh_clean_cpu as TC
from test_gpu_slam_session import sequence  # noqa: F401  (the fixture: six rendered frames of a hidden map)

pytestmark = pytest.mark.gpu

POISON, POISON64, TAIL = -77777, -7777777777, 8
B = R.BLOCK


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _poisoned(n, dtype=torch.int32, poison=POISON):
    return torch.full((n + TAIL,), poison, dtype=dtype, device=_device())


def components_once(faces, V):
    """hsr_mesh_components through the C ABI into poisoned buffers: (label, count) as numpy arrays"""
    from diff_gaussian_rasterization import _abi
    dev = _device()
    F = len(faces)
    f = torch.from_numpy(np.ascontiguousarray(faces, np.int32).reshape(F, 3)).to(dev)
    label, count = _poisoned(V), _poisoned(V)
    _abi.call(_abi.lib.hsr_mesh_components, "hsr_mesh_components", dev, V, F, f.data_ptr() if F else None, label.data_ptr() if V else None,
              count.data_ptr() if V else None)
    assert (label[V:] == POISON).all() and (count[V:] == POISON).all(), "written behind an output"
    return label[:V].cpu().numpy(), count[:V].cpu().numpy()


def select_once(faces, V, label, keep):
    """hsr_mesh_select through the C ABI into poisoned buffers: (faces [F',3], source [V']); everything behind F' and V' still poisoned"""
    from diff_gaussian_rasterization import _abi
    dev = _device()
    F = len(faces)
    f = torch.from_numpy(np.ascontiguousarray(faces, np.int32).reshape(F, 3)).to(dev)
    lab, kp = torch.from_numpy(np.ascontiguousarray(label, np.int32)).to(dev), torch.from_numpy(np.ascontiguousarray(keep, np.uint8)).to(dev)
    out_faces, source, counts = _poisoned(3 * F), _poisoned(V), _poisoned(3, torch.int64, POISON64)
    need = _abi.lib.hsr_mesh_select_scratch_bytes(V, F)
    scratch = torch.full((need + 16,), 0xA5, dtype=torch.uint8, device=dev)      # a dirty scratch: the call zeroes what it needs zeroed
    _abi.call(_abi.lib.hsr_mesh_select, "hsr_mesh_select", dev, V, F, f.data_ptr() if F else None, lab.data_ptr() if V else None,
              kp.data_ptr() if V else None, out_faces.data_ptr() if F else None, source.data_ptr() if V else None, counts.data_ptr(),
              scratch.data_ptr(), need)
    assert (scratch[need:] == 0xA5).all() and (counts[3:] == POISON64).all(), "written behind the scratch or the counts"
    nf, nv, gave_up = counts[:3].tolist()
    assert gave_up == 0 and 0 <= nf <= F and 0 <= nv <= V
    assert (out_faces[3 * nf:] == POISON).all() and (source[nv:] == POISON).all(), "written behind the kept rows"
    return out_faces[:3 * nf].cpu().numpy().reshape(nf, 3), source[:nv].cpu().numpy()


def check_components(faces, V):
    """twice on the device, both equal to the restatement; returns (label, count)"""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    want = R.components(faces, V)
    for _ in range(2):
        got = components_once(faces, V)
        assert (got[1] >= 0).all(), "a walk gave up"
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    return want


def check_select(faces, V, label, keep):
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    want = R.select(faces, V, label, keep)
    for _ in range(2):
        got = select_once(faces, V, label, keep)
        assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    return want


def check_both(faces, V, **rule):
    label, count = check_components(faces, V)
    return check_select(faces, V, label, R.keep(count, **rule))


# ---- trivial ----------------------------------------------------------------------------------------------------------------------------------
TRIVIAL = {
    "no_faces": ([], 5),
    "one_face": ([[2, 0, 1]], 3),
    "share_a_vertex": ([[0, 1, 2], [2, 3, 4]], 5),
    "share_an_edge": ([[4, 1, 2], [2, 1, 3]], 5),
    "disjoint": ([[5, 1, 2], [0, 3, 4]], 6),
    "repeated_index": ([[3, 3, 1], [2, 2, 2], [0, 4, 0]], 6),
    "index_of_minus_one_and_of_V": ([[0, 1, -1], [1, 2, 3], [6, 4, 5], [4, 5, 3], [0, 6, 1]], 6),
    "unreferenced": ([[7, 3, 5]], 9),
}


@pytest.mark.parametrize("name", sorted(TRIVIAL))
def test_trivial(name):
    faces, V = TRIVIAL[name]
    faces = np.array(faces, np.int32).reshape(-1, 3)
    label, count = check_components(faces, V)
    assert count.sum() == R.valid_faces(faces, V).sum()
    out, source = check_select(faces, V, label, R.keep(count))      # every component with a face
    assert len(out) == R.valid_faces(faces, V).sum() and len(source) == len(np.unique(faces[R.valid_faces(faces, V)]))
    check_select(faces, V, label, np.zeros(V, np.uint8))
    check_select(faces, V, label, R.keep(count, largest=True))


def test_no_vertices():
    from hsr_utils import mesh_clean
    label, count = components_once(np.zeros((0, 3), np.int32), 0)
    assert label.shape == count.shape == (0,)
    components_once(np.array([[0, 1, 2]], np.int32), 0)      # every face is invalid: nothing is written, nothing is read
    out, source = select_once(np.array([[0, 1, 2]], np.int32), 0, np.zeros(0, np.int32), np.zeros(0, np.uint8))
    assert out.shape == (0, 3) and source.shape == (0,)
    dev = _device()
    got = mesh_clean.clean_mesh(torch.zeros((0, 3), device=dev), torch.zeros((0, 3), dtype=torch.int32, device=dev),
                                torch.zeros((0, 3), dtype=torch.uint8, device=dev), None, min_faces=3)
    assert [None if t is None else (tuple(t.shape), t.dtype) for t in got] == [((0, 3), torch.float32), ((0, 3), torch.int32), ((0, 3), torch.uint8), None]


# ---- deep chains, contention ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numbering", ["ascending", "descending", "permuted"])
def test_deep_chains(numbering):
    faces, V = R.strip(3000, numbering)
    label, count = check_components(faces, V)
    assert (label == 0).all() and count[0] == 3000
    check_select(faces, V, label, R.keep(count, largest=True))


@pytest.mark.parametrize("hub", ["first", "last"])
def test_contention(hub):
    faces, V = R.fan(2000, hub)      # "last": every lane hooks the same root
    label, count = check_components(faces, V)
    assert (label == 0).all() and count[0] == 2000
    check_select(faces, V, label, R.keep(count))


# ---- many components and the seams of the compaction -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2 * B + 1, B - 1, B, B + 1, 3 * B - 1, 3 * B, 3 * B + 1])
def test_many_components_and_face_seams(n):
    faces, V = R.disjoint(n)      # n components of one face; V = 3 n
    label, count = check_components(faces, V)
    assert (count > 0).sum() == n
    keep = R.keep(count)
    keep[label[faces[::3, 0]]] = 0      # every third face goes: kept faces on both sides of every block border
    out, source = check_select(faces, V, label, keep)
    assert len(out) == n - len(faces[::3]) and len(source) == 3 * len(out)
    keep = np.zeros(V, np.uint8)
    ends = sorted({0, min(B, n) - 1, n - 1})      # the first face, the last of the first block, the last of all
    keep[label[faces[ends, 0]]] = 1
    assert len(check_select(faces, V, label, keep)[0]) == len(ends)


@pytest.mark.parametrize("V", [B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1])
def test_vertex_seams(V):
    rng = np.random.default_rng(V)
    faces = np.stack([np.arange(0, V - 2), np.arange(1, V - 1), np.arange(2, V)], axis=1)[::5]      # short runs with unreferenced vertices between
    faces = np.concatenate([faces, [[V - 1, V - 1, V - 1], [0, 0, 0]]]).astype(np.int32)             # the last vertex and the first are used
    faces = faces[rng.permutation(len(faces))]
    label, count = check_components(faces, V)
    out, source = check_select(faces, V, label, R.keep(count))
    assert source[0] == 0 and source[-1] == V - 1 and len(source) < V
    check_select(faces, V, label, R.keep(count, min_faces=2))


# ---- mixed ------------------------------------------------------------------------------------------------------------------------------------
def test_mixed_patches():
    faces, V, n = R.patches()
    label, count = check_components(faces, V)
    sizes = sorted(set(count[count > 0].tolist()))
    assert (count > 0).sum() == n == 36 and len(sizes) >= 10
    everything = check_select(faces, V, label, R.keep(count))
    assert len(everything[0]) == len(faces) and len(everything[1]) < V      # the unreferenced vertices go
    nothing = check_select(faces, V, label, np.zeros(V, np.uint8))
    assert nothing[0].shape == (0, 3) and nothing[1].shape == (0,)
    middle = (sizes[len(sizes) // 2 - 1] + sizes[len(sizes) // 2]) // 2 + 1      # between two patch sizes
    some = check_both(faces, V, min_faces=middle)
    assert 0 < len(some[0]) < len(faces)
    one = check_both(faces, V, largest=True)
    assert len(one[0]) == sizes[-1]
    check_both(faces, V, min_ratio=0.5)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------------
def test_python_layer_equals_the_restatement():
    from hsr_utils import mesh_clean
    faces, V, _n = R.patches(seed=3)
    dev = _device()
    f = torch.from_numpy(faces).to(dev)
    label, count = mesh_clean.mesh_components(f, V)
    want = R.components(faces, V)
    assert label.dtype == count.dtype == torch.int32 and np.array_equal(label.cpu().numpy(), want[0]) and np.array_equal(count.cpu().numpy(), want[1])
    keep = mesh_clean.component_keep(count, min_ratio=0.4)
    assert keep.device == count.device and np.array_equal(keep.cpu().numpy(), R.keep(want[1], min_ratio=0.4))
    vertices = torch.arange(3 * V, dtype=torch.float32, device=dev).reshape(V, 3)
    rgb = (torch.arange(3 * V, device=dev) % 251).to(torch.uint8).reshape(V, 3)
    labels = torch.arange(V, dtype=torch.int32, device=dev) * 3
    for rule in (dict(min_ratio=0.4), dict(largest=True), dict(min_faces=10 ** 6), dict()):
        v, fo, c, lab = mesh_clean.clean_mesh(vertices, f, rgb, labels, **rule)
        wv, wf, src = R.clean(vertices.cpu().numpy(), faces, **rule)
        assert (v.dtype, fo.dtype, c.dtype, lab.dtype) == (torch.float32, torch.int32, torch.uint8, torch.int32)
        assert fo.shape == wf.shape and np.array_equal(fo.cpu().numpy(), wf) and np.array_equal(v.cpu().numpy(), wv)
        assert np.array_equal(c.cpu().numpy(), rgb.cpu().numpy()[src]) and np.array_equal(lab.cpu().numpy(), labels.cpu().numpy()[src])
    v, fo, c, lab = mesh_clean.clean_mesh(vertices, f, min_faces=1)
    assert c is None and lab is None and len(fo) == len(faces)


# ---- end to end on a real extraction -------------------------------------------------------------------------------------------------------------
def _on_device(ref):
    from hsr_utils import mesh
    X, Y, Z = TC.DIMS
    vol = mesh.TsdfVolume(ref.origin, TC.DIMS, float(ref.h), trunc=float(ref.trunc), labels=True)
    for name in ("tsdf", "weight", "cweight", "label"):
        getattr(vol, name).copy_(torch.from_numpy(getattr(ref, name).reshape(Z, Y, X)))
    vol.color.copy_(torch.from_numpy(ref.color.reshape(3, Z, Y, X)))
    return vol


def test_cleaning_a_real_extraction_leaves_the_large_sphere_bit_for_bit():
    from hsr_utils import mesh_clean
    both, big = (_on_device(v) for v in TC.two_spheres())
    vertices, faces, rgb, labels = both.extract()
    want = big.extract()
    label, count = mesh_clean.mesh_components(faces, len(vertices))
    assert len(faces) == 2416 and sorted(count[count > 0].tolist()) == [184, 2232] and len(want[1]) == 2232
    got = mesh_clean.clean_mesh(vertices, faces, rgb, labels, min_faces=185)
    assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3]) and len(torch.unique(got[3])) > 100
    for rule in (dict(largest=True), dict(min_ratio=0.1)):
        again = mesh_clean.clean_mesh(vertices, faces, rgb, labels, **rule)
        assert all(torch.equal(a, b) for a, b in zip(again, got))
    kept_all = mesh_clean.clean_mesh(vertices, faces, rgb, labels, min_faces=184)      # nothing to drop: the extraction itself
    assert all(torch.equal(a, b) for a, b in zip(kept_all, (vertices, faces, rgb, labels)))


# ---- mesh_run -------------------------------------------------------------------------------------------------------------------------------------
VOXEL, EVERY = 0.08, 2


@pytest.fixture(scope="module")
def session(sequence):  # noqa: F811
    """the short session of tests/test_gpu_mesh_run.py: all six frames, 2 tracking and 2 mapping iterations a frame"""
    from hsr_utils import SlamSession
    cam, intrinsics, frames = sequence
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    config = TS._config(2)
    config["mapping"]["num_iters"] = 2
    s = SlamSession(config, intrinsics, torch.eye(4, device="cuda"), cam)
    for frame in frames:
        s.step(frame)
    return s


def test_mesh_run_with_and_without_the_keywords(session, tmp_path):
    from hsr_utils import mesh
    plain = session.export_mesh(str(tmp_path / "plain.ply"), voxel_size=VOXEL, every=EVERY)
    off = session.export_mesh(str(tmp_path / "off.ply"), voxel_size=VOXEL, every=EVERY, min_component_faces=0, min_component_ratio=0.0,
                              largest_component=False)
    assert off[1:] == plain[1:] and open(off[0], "rb").read() == open(plain[0], "rb").read()
    one = session.export_mesh(str(tmp_path / "one.ply"), voxel_size=VOXEL, every=EVERY, largest_component=True)
    v0, f0, _rgb0, _lab0 = mesh.load_mesh_ply(plain[0])
    v1, f1, rgb1, lab1 = mesh.load_mesh_ply(one[0])
    assert one[1:] == (len(v1), len(f1)) and len(f1) > 0 and rgb1 is not None and lab1 is not None
    label, count = R.components(f1, len(v1))
    assert (label == 0).all() and count[0] == len(f1)      # exactly one component, no unreferenced vertex
    # its faces are faces of the uncleaned file, in that file's order: by position, a vertex keeps its coordinates bit for bit
    want_v, want_f, src = R.clean(v0, f0, largest=True)
    assert np.array_equal(f1, want_f) and np.array_equal(v1.view(np.uint32), want_v.view(np.uint32))
    label0, count0 = R.components(f0, len(v0))
    kept = np.flatnonzero(label0[f0[:, 0]] == int(np.argmax(R.keep(count0, largest=True))))
    assert np.array_equal(src[f1], f0[kept])      # a subsequence of the uncleaned faces
    print("session mesh: %d faces in %d components, the largest %d" % (len(f0), (count0 > 0).sum(), len(f1)))
