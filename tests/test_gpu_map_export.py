"""GPU suite for hsr_utils.map_export / hsr_map_export (include/ext/hsr_map_export.h): every body is compared BIT FOR BIT with the numpy
restatement of the header, tests/map_export_ref.py (which tests/test_map_export_cpu.py ties to the host writers of hsr_utils.map_io byte
for byte); a NaN f_dc of the restatement asks for a NaN, whatever its payload.  The logits of every case lie on a grid of 1/64 (asserted
on the host by map_export_ref.tree_labels before use), so that the first index of a level's largest value is the header's label; the
levels holding a NaN or an infinity are asserted against the header's stated rule (label 0) instead.  Sizes: 1, 63, 64, 65 (around a
wave), 255, 256, 257 (around a workgroup) and 1000 Gaussians."""
import ctypes as C

import numpy as np
import pytest
import torch

import map_export_ref as R
import test_map_export_cpu as RC
from test_gpu_slam_session import sequence  # noqa: F401  (the fixture: that suite's synthetic sequence)

pytestmark = pytest.mark.gpu

SIZES26, K26 = (4, 8, 14), 26


def _dev(a, offset=0):
    """the array on the device; with offset, as a view `offset` elements into a larger allocation: same values, a pointer off 16 bytes"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.cuda()
    big = torch.empty(t.numel() + offset, dtype=t.dtype, device="cuda")
    view = big[offset:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


def _params(m, offset=0):
    return {k: _dev(v, offset) for k, v in m.items() if k != "normals"}


def _tables(n_tuples, seed=4):
    from hsr_utils.export import label_colormap
    g = np.random.default_rng(seed)
    return label_colormap(40, "cpu").numpy(), g.integers(1, 256, size=(n_tuples, 3)).astype(np.uint8)      # no black tuple: black means refused


def _labels(P):
    return R.X.lay(np.array([0, 39, 40, -1, 7, 2 ** 31 - 1, -2 ** 31, 12, 38, 1], dtype=np.int32), (P,))


@pytest.mark.parametrize("with_normals", [False, True], ids=["zeros", "normals"])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("P", R.COUNTS)
def test_bodies_match_the_restatement_bit_for_bit(P, S, with_normals):
    """both record kinds and all four colour sources, on rgb_colors holding 0, 0.5, 1, the floats either side of 0.5, denormals, the
    infinities and NaN, and copied arrays holding NaNs of three payloads"""
    from hsr_utils.map_export import FIELDS_RGB8, FIELDS_SH, export_map
    m = R.make_map(P, S, K26, 100 * S + P)
    class_table, tuple_table = _tables(int(np.prod(SIZES26)))
    given = np.random.default_rng(P).integers(0, 256, size=(P, 3)).astype(np.uint8)
    lab = _labels(P)
    normals = m["normals"] if with_normals else None
    params = _params(m)
    kw = dict(normals=None if normals is None else _dev(normals))
    body, fields = export_map(params, **kw)
    assert body.dtype == torch.uint8 and body.is_contiguous() and tuple(body.shape) == (P * 68,) and list(fields) == [tuple(f) for f in R.FIELDS_SH]
    assert fields is FIELDS_SH
    R.same_body(body.cpu().numpy(), R.body_sh(m, normals), 68)
    want = {"given": given, "labels": R.colours_labels(lab, class_table), "tree": R.colours_tree(m["semantic"], SIZES26, tuple_table)}
    got = {
        "given": export_map(params, colour="given", colours=_dev(given), **kw),
        "labels": export_map(params, colour="labels", labels=_dev(lab), table=_dev(class_table), **kw),
        "tree": export_map(params, colour="tree", table=_dev(tuple_table), level_sizes=list(SIZES26) + [99], **kw),
    }
    for name in want:
        body, fields = got[name]
        assert tuple(body.shape) == (P * 59,) and fields is FIELDS_RGB8
        R.same_body(body.cpu().numpy(), R.body_rgb8(m, want[name], normals), 59)
    if P == 1000:
        assert want["tree"].any(axis=1).all() and not want["labels"].any(axis=1).all()      # every tuple found a colour; some labels are refused


def _rule_labels(x, sizes):
    """the header's labels where a level may hold a NaN or an infinity: 0 by the stated rule where it holds a NaN or +inf (the sum is then
    a NaN and no quotient equals 1 / s); a -inf beside finite values is a value like any other, far below them"""
    clean = np.where(np.isfinite(x), x, np.float32(0))
    clean[np.isneginf(x)] = -1000.0
    want = R.tree_labels(clean, sizes)
    begin = 0
    for l, s in enumerate(sizes):
        bad = (np.isnan(x[:, begin:begin + s]) | np.isposinf(x[:, begin:begin + s])).any(axis=1)
        want[l, bad] = 0
        begin += s
    return want


# the level sets of the datasets (1, 2, 3 and 5 levels, K = 26 and 102) and 16 levels of one class, then one K for every way the kernel
# reads the rows: workgroups of 4 waves (K = 26), 2 (K = 60, 102) and 1 (K = 200) with 64 rows staged per wave, and the rows read from
# global memory (K = 400)
LABEL_CASES = [((1,), 1), ((2, 3), 5), ((4, 8, 14), 26), ((3, 5, 9, 17, 68), 102), ((1,) * 16, 16), ((4, 8, 14), 31), ((7, 20, 30), 60),
               ((50, 100, 45), 200), ((3, 390), 400)]


@pytest.mark.parametrize("sizes,K", LABEL_CASES, ids=["%dx%d" % (len(s), k) for s, k in LABEL_CASES])
def test_tree_labels_match_the_rule(sizes, K):
    """gaussian_tree_labels and the labels returned beside a body: exact ties (the first index wins), columns past the levels that hold
    NaNs, a level of all NaN and a level holding +inf (label 0 by the header's rule, not np.argmax's)"""
    from hsr_utils.map_export import export_map, gaussian_tree_labels
    P = 300
    m = R.make_map(P, 1, K, K)
    x = m["semantic"]
    used = sum(sizes)
    x[:, used:] = np.nan                                            # never read
    x[::7, :used] = 1.5                                             # every column equal: label 0 on every level
    begin = 0
    for s in sizes:
        if s >= 3:
            x[1::7, begin:begin + s] = -2.0
            x[1::7, [begin + 1, begin + s - 1]] = 0.75              # two columns tie for the maximum: the lower one wins
        begin += s
    last = used - sizes[-1]
    x[2::11, last:used] = np.nan                                    # a level of all NaN
    x[3::11, last] = np.inf                                         # a level holding +inf
    x[5::11, 0] = -np.inf                                           # and one holding -inf: its column never wins
    want = _rule_labels(x, sizes)
    assert (want[-1, 2::11] == 0).all() and (want[-1, 3::11] == 0).all() and (sizes[0] == 1 or (want[0, 5::11] > 0).all())
    if max(sizes) >= 3:
        assert (want[:, 1::7] > 0).any() and len(np.unique(want)) > 2
    level_sizes = list(sizes) + [7]
    sem = _dev(x)
    got = gaussian_tree_labels(sem, level_sizes)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(sizes), P)
    assert np.array_equal(got.cpu().numpy(), want)
    n = int(np.prod(sizes))
    if n <= 1 << 20:
        table = np.random.default_rng(K).integers(1, 256, size=(n, 3)).astype(np.uint8)
        params = _params(m)
        params["semantic"] = sem
        body, _fields, beside = export_map(params, colour="tree", table=_dev(table), level_sizes=level_sizes, return_labels=True)
        assert torch.equal(beside, got)
        R.same_body(body.cpu().numpy(), R.body_rgb8(m, R.X.levels(want[:, None, :], sizes, table)[0], None), 59)
    off = gaussian_tree_labels(_dev(x, 1), level_sizes)             # a pointer off 16 bytes: the narrow variant
    assert torch.equal(off, got)


def test_tree_labels_are_those_of_semantic_labels_bit_for_bit():
    """on logits with near ties that only the fp32 softmax decides: hsr_eval_labels_tree on the transposed logits gives the same labels"""
    from hsr_utils import evaluate
    from hsr_utils.map_export import gaussian_tree_labels
    P, sizes = 5000, (3, 5, 8, 6)
    g = np.random.default_rng(17)
    x = (g.normal(size=(P, K26)) * 3).astype(np.float32)
    x[::3, 1] = x[::3, 0] + np.float32(3e-8)                         # within the 1e-6 pre-test: expf and the division decide
    x[1::3, 9] = np.maximum(x[1::3, 8], x[1::3, 10]) + np.float32(5e-7)
    x[2::5, 16:22] = x[2::5, 16:17]
    x[3::11, 8:16] = np.float32(80.0) * np.arange(8, dtype=np.float32)      # differences that underflow expf
    x[:, 22:] = np.nan
    level_sizes = list(sizes) + [99]
    sem = _dev(x)
    planes = sem.t().contiguous().view(K26, 1, P)
    _leaf, levels = evaluate.semantic_labels(planes, "tree", level_sizes=level_sizes,
                                             tree_table=torch.zeros(int(np.prod(sizes)), dtype=torch.int32, device="cuda"))
    assert torch.equal(gaussian_tree_labels(sem, level_sizes), levels.view(len(sizes), P))


@pytest.fixture(scope="module")
def mapped():
    """the map of 8 000 Gaussians that tests/test_gpu_map_io.py optimises on the device, its logits rounded to the grid of 1/64"""
    from test_gpu_map_io import _mapped_scene
    _cam, params, _whk = _mapped_scene(iters=2)
    params = dict(params)
    params["semantic"] = (torch.round(params["semantic"] * 64) / 64).contiguous()
    return params, {k: v.cpu().numpy() for k, v in params.items()}


def test_files_equal_the_host_writers_byte_for_byte(tmp_path, mapped):
    from hsr_utils import map_io
    from hsr_utils.export import tuple_colour_table
    from hsr_utils.map_export import save_map_ply, save_map_ply_semantic
    params, host = mapped
    P = host["means3D"].shape[0]
    assert P == 8000 and host["log_scales"].shape == (P, 1) and host["semantic"].shape[1] == 12
    args = (host["means3D"], host["log_scales"], host["unnorm_rotations"])
    mine = save_map_ply(str(tmp_path / "map.ply"), params)
    theirs = map_io.save_ply(str(tmp_path / "map_host.ply"), *args, host["rgb_colors"], host["logit_opacities"])
    assert open(mine, "rb").read() == open(theirs, "rb").read()
    level_sizes = [4, 8, 20]
    g = np.random.default_rng(12)
    colour_map = {(a, b): tuple(int(v) for v in g.integers(1, 256, size=3)) for a in range(4) for b in range(8) if (a + b) % 5}
    colour_map[(2, -1)] = (9, 8, 7)
    for wildcard in (True, False):
        table = tuple_colour_table(colour_map, level_sizes, wildcard, device="cpu").numpy()
        labels = map_io.transfer_tree_label(host["semantic"], level_sizes)
        R.assert_separated(host["semantic"], level_sizes[:-1])
        colours = table[labels[0] * 8 + labels[1]]
        assert colours.any(axis=1).any() and not colours.any(axis=1).all()
        mine = save_map_ply_semantic(str(tmp_path / "sem.ply"), params, colour_map, level_sizes, wildcard=wildcard)
        theirs = map_io.save_ply_semantic(str(tmp_path / "sem_host.ply"), *args, colours, host["logit_opacities"])
        assert open(mine, "rb").read() == open(theirs, "rb").read()
    a, b = map_io.read_ply(mine), map_io.read_ply(theirs)
    assert a.dtype == b.dtype and a.dtype.itemsize == 59 and len(a) == P
    for name in a.dtype.names:
        assert np.array_equal(a[name], b[name]), name
    # the leaf-head colouring: class ids from evaluate.semantic_labels on the logits viewed as [K,1,P], then the class table
    from hsr_utils.export import label_colormap
    from hsr_utils.map_export import leaf_head_labels
    gen = torch.Generator().manual_seed(3)
    weight, bias = torch.randn(20, 12, generator=gen).cuda(), torch.randn(20, generator=gen).cuda()
    ids = leaf_head_labels(params["semantic"], (weight, bias))
    assert ids.dtype == torch.int32 and tuple(ids.shape) == (P,) and len(torch.unique(ids)) > 3
    cmap = label_colormap(20, "cuda")
    mine = save_map_ply_semantic(str(tmp_path / "leaf.ply"), params, None, None, wildcard=False, labels=ids, table=cmap)
    theirs = map_io.save_ply_semantic(str(tmp_path / "leaf_host.ply"), *args, cmap.cpu().numpy()[ids.cpu().numpy()], host["logit_opacities"])
    assert open(mine, "rb").read() == open(theirs, "rb").read()


@pytest.mark.parametrize("i_level", [0, 1, 2])
def test_exporting_a_level_colours_as_the_reference_does(tmp_path, i_level):
    from hsr_utils import map_io
    from hsr_utils.export import label_colormap
    from hsr_utils.map_export import save_map_ply_semantic
    sizes = RC.TREE_SIZES
    P = 700
    m = R.make_map(P, 3, sum(sizes[:-1]) + 2, 60 + i_level)
    levels = R.tree_labels(m["semantic"], sizes[:-1])
    mapping = RC.TREE_ID_CLASSES_MAP[i_level]
    colours = R.multilevel_colours_literal(torch.from_numpy(levels[:i_level + 1]), mapping, lambda n: label_colormap(n, "cpu").numpy())
    assert len(np.unique(colours, axis=0)) >= len(mapping) - 1
    path = save_map_ply_semantic(str(tmp_path / "level.ply"), _params(m), None, sizes, wildcard=False, i_level=i_level,
                                 tree_id_classes_map_level=mapping)
    raw = open(path, "rb").read()
    head = R.header(P, R.FIELDS_RGB8)
    assert raw[:len(head)] == head
    R.same_body(np.frombuffer(raw[len(head):], dtype=np.uint8), R.body_rgb8(m, colours, None), 59)
    el = map_io.read_ply(path)
    assert np.array_equal(np.stack([el["red"], el["green"], el["blue"]], axis=1), colours)


# ---- the raw entry point: alignment, bounds, refusals ----------------------------------------------------------------------------------
CANARY, PAD = 0xA5, 64


def _raw_job(m, dev, record, colour=0, sizes=(), out_offset=0, table=None, extra=None):
    """the job of one raw call over device tensors `dev` (a dict), its output `out_offset` bytes into a canary-filled buffer"""
    from diff_gaussian_rasterization import _abi
    P = m["means3D"].shape[0]
    stride = {0: 68, 1: 59, 2: 0}[record]
    buf = torch.full((PAD + P * stride + PAD,), CANARY, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    job = _abi.hsr_map_export_job(P=P, S=m["log_scales"].shape[1], record=record, colour=colour, out=buf.data_ptr() + PAD + out_offset)
    for name in ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales", "normals", "semantic", "colours", "labels"):
        if name in dev:
            setattr(job, name, dev[name].data_ptr())
    if sizes:
        job.K, job.L = m["semantic"].shape[1], len(sizes)
        job.sizes[:len(sizes)] = list(sizes)
    if table is not None:
        job.table, job.n = table.data_ptr(), table.shape[0]
    for k, v in (extra or {}).items():
        setattr(job, k, v)
    return job, buf


def _run_raw(job, buf, P, stride, out_offset):
    from diff_gaussian_rasterization import _abi
    _abi.call(_abi.lib.hsr_map_export, "hsr_map_export", buf.device, C.byref(job))
    got = buf.cpu().numpy()
    lo, hi = PAD + out_offset, PAD + out_offset + P * stride
    assert (got[:lo] == CANARY).all() and (got[hi:] == CANARY).all(), "a byte outside the body was written"
    return got[lo:hi]


@pytest.mark.parametrize("record,colour", [(0, 0), (1, 0), (1, 1), (1, 2)], ids=["sh", "given", "labels", "tree"])
def test_alignment_and_bounds_through_the_entry_point(record, colour):
    """P = 257: the tail workgroup holds one Gaussian.  `out` 0, 1, 2, 3 and 8 bytes into a canary-filled buffer, then every input one
    element into its allocation: the same bytes, and no byte before the body or after P * stride touched"""
    P, stride = 257, 68 if record == 0 else 59
    m = R.make_map(P, 3, K26, 7)
    m["colours"] = np.random.default_rng(1).integers(0, 256, size=(P, 3)).astype(np.uint8)
    m["labels"] = _labels(P)
    class_table, tuple_table = _tables(int(np.prod(SIZES26)))
    table = _dev(class_table if colour == 1 else tuple_table)
    want = R.body_sh(m, m["normals"]) if record == 0 else R.body_rgb8(
        m, [m["colours"], R.colours_labels(m["labels"], class_table), R.colours_tree(m["semantic"], SIZES26, tuple_table)][colour], m["normals"])
    sizes = SIZES26 if colour == 2 and record == 1 else ()
    aligned = {k: _dev(v) for k, v in m.items()}
    for out_offset in (0, 1, 2, 3, 8):
        job, buf = _raw_job(m, aligned, record, colour, sizes, out_offset, table)
        R.same_body(_run_raw(job, buf, P, stride, out_offset), want, stride)
    shifted = {k: _dev(v, 1) for k, v in m.items()}
    for out_offset in (0, 3):
        job, buf = _raw_job(m, shifted, record, colour, sizes, out_offset, table)
        R.same_body(_run_raw(job, buf, P, stride, out_offset), want, stride)
    # one input alone off 16 bytes is enough to take the narrow variant
    one = dict(aligned)
    one["unnorm_rotations"] = shifted["unnorm_rotations"]
    job, buf = _raw_job(m, one, record, colour, sizes, 0, table)
    R.same_body(_run_raw(job, buf, P, stride, 0), want, stride)


@pytest.mark.parametrize("base", list(RC.BASES))
def test_refusals_leave_the_outputs_untouched(base):
    """every refusal of the header (the list of the CPU suite, here with device pointers and a valid job of each kind as the base): the
    error code, the message, and the canary-filled outputs unchanged; then the base itself writes every byte"""
    from diff_gaussian_rasterization import _abi
    P = 8
    out = torch.full((P * 68,), CANARY, dtype=torch.uint8, device="cuda")
    out_labels = torch.full((16 * P,), -1515870811, dtype=torch.int32, device="cuda")      # 0xA5A5A5A5
    src = torch.zeros(64 * P, dtype=torch.float32, device="cuda")                         # zeros are valid input of every kind
    table = torch.ones((256, 3), dtype=torch.uint8, device="cuda")
    kw = dict(RC.BASES[base], P=P)
    kw.update({name: src.data_ptr() for name in RC.POINTERS})
    kw.update(table=table.data_ptr(), out=out.data_ptr(), out_labels=out_labels.data_ptr())
    refused = 0
    with torch.cuda.device(out.device):
        for b, overrides, message in RC.REFUSALS:
            if b != base:
                continue
            rc = RC.refused_call(_abi.lib, kw, overrides)
            assert rc == -1 and message in _abi.lib.hsr_last_error(), (overrides, rc, _abi.lib.hsr_last_error())
            refused += 1
        torch.cuda.synchronize()
        assert bool((out == CANARY).all()) and bool((out_labels == -1515870811).all()) and refused >= 9
        assert RC.refused_call(_abi.lib, kw, {}) == 0
        torch.cuda.synchronize()
    stride = {"sh": 68, "none": 0}.get(base, 59)
    assert not bool((out[:P * stride] == CANARY).any()) and bool((out[P * stride:] == CANARY).all())
    written = 3 * P if base in ("tree", "none") else 0
    assert not bool((out_labels[:written] == -1515870811).any()) and bool((out_labels[written:] == -1515870811).all())


def test_an_empty_map_writes_a_header_only_file(tmp_path):
    from hsr_utils.map_export import export_map, gaussian_tree_labels, save_map_ply, save_map_ply_semantic
    m = R.make_map(0, 1, K26, 1)
    params = _params(m)
    body, fields = export_map(params)
    assert tuple(body.shape) == (0,) and len(fields) == 17
    assert open(save_map_ply(str(tmp_path / "empty.ply"), params), "rb").read() == R.header(0, R.FIELDS_SH)
    colour_map = {(0, 0, 0): (1, 2, 3)}
    path = save_map_ply_semantic(str(tmp_path / "empty_sem.ply"), params, colour_map, list(SIZES26) + [9], wildcard=False)
    assert open(path, "rb").read() == R.header(0, R.FIELDS_RGB8)
    assert tuple(gaussian_tree_labels(params["semantic"], list(SIZES26) + [9]).shape) == (3, 0)


def test_wrapper_checks_launch_nothing_and_one_call_is_one_launch(monkeypatch):
    from hsr_utils import map_export as M
    calls = []
    real = M._lib.hsr_map_export
    monkeypatch.setattr(M._lib, "hsr_map_export", lambda *a: calls.append(a) or real(*a))
    m = R.make_map(40, 1, K26, 2)
    params = _params(m)
    _class_table, tuple_table = _tables(int(np.prod(SIZES26)))
    with pytest.raises(RuntimeError, match=r"unnorm_rotations must be \[40,4\]"):
        M.export_map(dict(params, unnorm_rotations=params["unnorm_rotations"][:, :3]))
    with pytest.raises(RuntimeError, match="must be torch.float32"):
        M.export_map(dict(params, means3D=params["means3D"].double()))
    with pytest.raises(RuntimeError, match="needs colours"):
        M.export_map(params, colour="given")
    with pytest.raises(RuntimeError, match="colours must be"):
        M.export_map(params, colour="given", colours=torch.zeros(39, 3, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="level_sizes and table"):
        M.export_map(params, colour="tree", table=_dev(tuple_table))
    with pytest.raises(RuntimeError, match="table must be uint8"):
        M.export_map(params, colour="tree", table=_dev(tuple_table), level_sizes=[4, 8, 13, 9])
    with pytest.raises(RuntimeError, match="K >= 27"):
        M.export_map(params, colour="tree", table=_dev(tuple_table), level_sizes=[4, 8, 15, 9])
    assert calls == []
    # views that are not contiguous, and parameters that require grad, are taken as they are
    wide = torch.zeros(40, 8, device="cuda")
    wide[:, 2:5] = params["means3D"]
    loose = dict(params, means3D=wide[:, 2:5], rgb_colors=torch.nn.Parameter(params["rgb_colors"]), ignored="anything")
    body, _fields = M.export_map(loose)
    assert len(calls) == 1
    R.same_body(body.cpu().numpy(), R.body_sh(m), 68)
    body, _fields, labels = M.export_map(params, colour="tree", table=_dev(tuple_table), level_sizes=list(SIZES26) + [9], return_labels=True)
    assert len(calls) == 2 and tuple(labels.shape) == (3, 40)


def test_session_exports_its_map(tmp_path, sequence):  # noqa: F811
    """SlamSession.export_map on a session stepped through the first two frames of tests/test_gpu_slam_session.py's synthetic sequence"""
    import test_gpu_slam_session as TS
    from hsr_utils import SlamSession, map_io
    from hsr_utils.export import tuple_colour_table
    cam, intrinsics, frames = sequence
    torch.manual_seed(0); np.random.seed(0)
    s = SlamSession(TS._config(2), intrinsics, torch.eye(4, device="cuda"), cam)
    with pytest.raises(RuntimeError, match="no map yet"):
        s.export_map(str(tmp_path / "none.ply"))
    for frame in frames[:2]:
        s.step(frame)
    P = int(s.params["means3D"].shape[0])
    el = map_io.read_ply(s.export_map(str(tmp_path / "session.ply")))
    assert len(el) == P > 1000 and el.dtype.itemsize == 68
    assert np.array_equal(el["x"], s.params["means3D"].detach()[:, 0].cpu().numpy())
    assert np.array_equal(el["scale_2"], s.params["log_scales"].detach()[:, 0].cpu().numpy())
    table = tuple_colour_table({(0, 0): (255, 0, 0), (0, 1): (0, 255, 0), (1, -1): (0, 0, 255)}, TS.LEVELS + [4], True)
    el = map_io.read_ply(s.export_map(str(tmp_path / "session_sem.ply"), colour="tree", table=table, level_sizes=TS.LEVELS + [4]))
    assert len(el) == P and el.dtype.itemsize == 59
    colours = np.stack([el["red"], el["green"], el["blue"]], axis=1).astype(np.int64)
    assert (colours.sum(axis=1) == 255).all() and len(np.unique(colours, axis=0)) == 3
