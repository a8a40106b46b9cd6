"""GPU suite for hsr_utils.frames.ingest_frame_planes / hsr_frame_ingest_planes (include/ext/hsr_frame_ingest_planes.h): every output is
compared BIT FOR BIT with the numpy restatement tests/ingest_planes_ref.py, which applies the rules of tests/ingest_ref.py to each
image's own size and adds the leaf-column rule.  Colour and depth are compared as int32 words, labels as int64; the one exception is a
NaN depth (float32 input), which must be a NaN where the restatement has one.  Every case also runs the C entry itself on outputs
that sit inside sentinel-filled buffers: the words before and after each output must keep the sentinel."""
import functools

import numpy as np
import pytest
import torch

import ingest_planes_ref as P
import ingest_ref as I

pytestmark = pytest.mark.gpu

GUARD = 97                      # words of sentinel on either side of every output of the direct calls
FILL, LABEL_FILL = -7.25, -99
N_IDS = 12                      # rows of the label tables of the small cases

# (colour, depth, labels) sizes -> output sizes
SHAPES = {
    "1x1": ((1, 1), (1, 1), (1, 1), [(1, 1)]),
    "three-sizes": ((7, 9), (3, 5), (11, 4), [(3, 5), (5, 7), (2, 2)]),             # level 0 is the depth's size: identity index
    "scannet-tenth": ((97, 130), (48, 64), (97, 130), [(48, 64), (24, 32)]),        # ScanNet's 2.02 ratio at a tenth
    "depth-larger": ((5, 6), (33, 47), (5, 6), [(16, 20)]),
}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_depth(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _ids(shape, seed):
    """int32 class ids: most inside a table of N_IDS rows, some negative, some beyond it"""
    g = np.random.default_rng(seed)
    ids = g.integers(-2, N_IDS + 4, size=shape).astype(np.int32)
    ids.reshape(-1)[:3] = (N_IDS - 1, -1, N_IDS)[:ids.size]
    return ids


def _table(L, leaf, seed=5, n_ids=N_IDS):
    """int32 [n_ids, L + leaf] with -1 entries, or None without a column"""
    if L + int(leaf) == 0:
        return None
    table = np.random.default_rng(seed).integers(-1, 40, size=(n_ids, L + int(leaf))).astype(np.int32)
    table[3] = -1
    return table


@functools.lru_cache(maxsize=None)
def _case(name):
    """(colour uint8, depth uint16, ids int32) of a SHAPES entry, and the restatement of the case with a 2-level + leaf table"""
    hc, hd, hl, sizes = SHAPES[name]
    col, _d = I.make_frame(*hc, seed=100 * hc[0] + hc[1])
    _c, dep = I.make_frame(*hd, seed=100 * hd[0] + hd[1] + 1)
    ids = _ids(hl, seed=hl[0])
    table = _table(2, True)
    return col, dep, ids, table, P.frame(col, dep, sizes, 1000.0, ids, table, True)


def _check(levels, labels, want_levels, want_labels):
    assert len(levels) == len(want_levels)
    for (c, d), (wc, wd) in zip(levels, want_levels):
        assert c.dtype == d.dtype == torch.float32 and c.is_contiguous() and d.is_contiguous()
        assert tuple(c.shape) == wc.shape and tuple(d.shape) == (1,) + wd.shape
        assert np.array_equal(_bits(c.cpu().numpy()), _bits(wc))
        assert _same_depth(d.cpu().numpy()[0], wd)
    if want_labels is None:
        assert labels is None
    else:
        assert labels.dtype == torch.int64 and labels.is_contiguous() and tuple(labels.shape) == want_labels.shape
        assert np.array_equal(labels.cpu().numpy(), want_labels)


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _entry(col, dep, depth_type, scale, ids, table, leaf, sizes, over=()):
    """hsr_frame_ingest_planes itself on device tensors, every output inside a sentinel-filled buffer: (rc, [(colour, depth) views],
    label view | None, all buffers with their fills).  `over` (a dict) replaces arguments of the call by name."""
    from diff_gaussian_rasterization import _abi
    bufs, views = [], []
    for h, w in sizes:
        cb, cv = _guarded(3 * h * w, torch.float32, FILL)
        db, dv = _guarded(h * w, torch.float32, FILL)
        bufs += [(cb, FILL), (db, FILL)]
        views.append((cv, dv))
    L = 0 if table is None else int(table.shape[1]) - int(leaf)
    lv = None
    if ids is not None:
        lb, lv = _guarded((L + 1) * sizes[0][0] * sizes[0][1], torch.int64, LABEL_FILL)
        bufs.append((lb, LABEL_FILL))
    a = dict(Hc=col.shape[0], Wc=col.shape[1], Hd=dep.shape[0], Wd=dep.shape[1], depth_type=depth_type, scale=scale,
             Hl=0 if ids is None else ids.shape[0], Wl=0 if ids is None else ids.shape[1], L=L,
             table=None if table is None else table.data_ptr(), n_ids=0 if table is None else int(table.shape[0]), leaf=int(leaf),
             n_out=len(sizes), level_sizes=list(sizes))
    a.update(dict(over))
    arr = (_abi.hsr_ingest_level * len(views))(*[_abi.hsr_ingest_level(h, w, c.data_ptr(), d.data_ptr()) for (h, w), (c, d) in zip(a["level_sizes"], views)])
    with torch.cuda.device(col.device):
        rc = _abi.lib.hsr_frame_ingest_planes(a["Hc"], a["Wc"], col.data_ptr(), a["Hd"], a["Wd"], dep.data_ptr(), a["depth_type"], a["scale"],
                                              a["Hl"], a["Wl"], None if ids is None else ids.data_ptr(), a["L"], a["table"], a["n_ids"],
                                              a["leaf"], a["n_out"], arr, None if lv is None else lv.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, views, lv, bufs


def _guards_intact(bufs):
    return all(bool((b[:GUARD] == fill).all()) and bool((b[-GUARD:] == fill).all()) for b, fill in bufs)


def _direct_equals(levels, labels, views, lv, sizes):
    """the direct call's outputs are the wrapper's, word for word"""
    for (c, d), (cv, dv) in zip(levels, views):
        assert torch.equal(c.reshape(-1).view(torch.int32), cv.view(torch.int32)) and torch.equal(d.reshape(-1).view(torch.int32), dv.view(torch.int32))
    assert (labels is None) == (lv is None) and (labels is None or torch.equal(labels.reshape(-1), lv))


@pytest.mark.parametrize("name", list(SHAPES))
def test_planes_match_the_restatement_bit_for_bit(name):
    from hsr_utils import ingest_frame_planes
    sizes = SHAPES[name][3]
    col, dep, ids, table, (want_levels, want_labels) = _case(name)
    col_d, dep_d, ids_d, table_d = (torch.from_numpy(col).cuda(), torch.from_numpy(dep.view(np.int16)).cuda(), torch.from_numpy(ids).cuda(),
                                    torch.from_numpy(table).cuda())
    levels, labels = ingest_frame_planes(col_d, dep_d, sizes, 1000.0, labels=ids_d, label_table=table_d, leaf_column=True)
    _check(levels, labels, want_levels, want_labels)
    rc, views, lv, bufs = _entry(col_d, dep_d, 0, 1000.0, ids_d, table_d, True, sizes)
    assert rc == 0 and _guards_intact(bufs)
    _direct_equals(levels, labels, views, lv, sizes)
    # without labels: the same colour and depth, nothing else
    levels, labels = ingest_frame_planes(col_d, dep_d, sizes, 1000.0)
    _check(levels, labels, want_levels, None)
    rc, views, lv, bufs = _entry(col_d, dep_d, 0, 1000.0, None, None, False, sizes)
    assert rc == 0 and lv is None and _guards_intact(bufs)
    _direct_equals(levels, None, views, None, sizes)
    if name == "three-sizes":      # the depth image has level 0's size: the index is the identity, the value word / scale exactly
        assert np.array_equal(want_levels[0][1], (dep.astype(np.float64) / 1000.0).astype(np.float32))


@pytest.mark.parametrize("scale", (6553.5, 1000.0, 1.0))
@pytest.mark.parametrize("kind", ["uint16", "int16-bits", "int32", "float32"])
def test_depth_types_and_scales(kind, scale):
    from hsr_utils import ingest_frame_planes
    sizes = [(9, 11), (19, 23), (4, 3)]      # the depth's own size, a smaller and a larger one than the colour's
    col, _d = I.make_frame(13, 8, seed=3)
    _c, dep16 = I.make_frame(19, 23, seed=4)
    if kind in ("uint16", "int16-bits"):
        raw = dep16.copy()
        raw[1, :4] = (0, 65535, 32768, 32767)      # the sign bit of the int16 view is part of the value
        given, depth_type = (raw if kind == "uint16" else torch.from_numpy(raw.view(np.int16))), 0
        on_device = torch.from_numpy(raw.view(np.int16)).cuda()
    elif kind == "int32":
        raw = dep16.astype(np.int32) * 30000
        raw[1, :4] = (0, 2 ** 31 - 1, -5, 65536)
        given, depth_type = torch.from_numpy(raw).cuda(), 1
        on_device = given
    else:
        raw = dep16.astype(np.float32) * np.float32(0.37)
        raw[1, :5] = (np.nan, np.inf, 0.0, -np.inf, 1e-30)
        raw[5:9, 3:9] = 0.0
        given, depth_type = torch.from_numpy(raw), 2
        on_device = given.cuda()
    levels, labels = ingest_frame_planes(col, given, sizes, scale)
    want, _none = P.frame(col, raw, sizes, scale)
    _check(levels, labels, want, None)
    full = levels[1][1].cpu().numpy()[0]      # the level of the depth's own size
    if kind == "float32":
        assert np.isnan(full[1, 0]) and full[1, 1] == np.inf and full[1, 2] == 0.0 and full[1, 3] == -np.inf and not full[5:9, 3:9].any()
    elif kind != "int32":
        assert full[1, 0] == 0.0 and full[1, 1] == np.float32(65535.0 / scale) and full[1, 2] == np.float32(32768.0 / scale)
    rc, views, lv, bufs = _entry(torch.from_numpy(col).cuda(), on_device, depth_type, scale, None, None, False, sizes)
    assert rc == 0 and _guards_intact(bufs)
    _direct_equals(levels, None, views, None, sizes)


@pytest.mark.parametrize("leaf", [False, True], ids=["raw-id-plane", "leaf-column"])
@pytest.mark.parametrize("L", [0, 1, 5, 16])
def test_label_planes(L, leaf):
    from hsr_utils import ingest_frame_planes
    sizes = [(17, 33), (4, 4)]      # the labels follow level 0; their own size is neither the colour's nor the depth's
    col, _d = I.make_frame(9, 14, seed=6)
    _c, dep = I.make_frame(6, 5, seed=7)
    wide = _ids((33, 65), seed=8).astype(np.int64)
    wide[0, :6] = (-1, N_IDS, 1 << 40, (1 << 40) + 5, -(1 << 33) - 1, 3)      # int64 ids travel as int32: the wrapper keeps the low word
    ids = wide.astype(np.int32)
    assert ids[0, :6].tolist() == [-1, N_IDS, 0, 5, -1, 3]
    table = _table(L, leaf)
    table_d = None if table is None else torch.from_numpy(table).cuda()
    levels, labels = ingest_frame_planes(col, dep, sizes, 1000.0, labels=wide, label_table=table_d, leaf_column=leaf)
    want_levels, want = P.frame(col, dep, sizes, 1000.0, ids, table, leaf)
    assert want.shape == (L + 1, 17, 33)
    _check(levels, labels, want_levels, want)
    raw = I.labels(ids, sizes[0], None)[0]
    unknown = (raw < 0) | (raw >= N_IDS)
    assert unknown.any() and (raw == 3).any()
    assert all(np.array_equal(want[l][unknown], raw[unknown]) for l in range(L + 1))      # an id no row holds: the raw id on every plane
    if table is None or not leaf:
        assert np.array_equal(want[L], raw)                                               # the last plane is the raw id
    else:
        assert np.array_equal(want[L][~unknown], table[raw[~unknown], L].astype(np.int64)) and (want[L][raw == 3] == -1).all()
    if L:
        assert (want[:L][:, raw == 3] == -1).all()
    col_d, dep_d, ids_d = torch.from_numpy(col).cuda(), torch.from_numpy(dep.view(np.int16)).cuda(), torch.from_numpy(ids).cuda()
    rc, views, lv, bufs = _entry(col_d, dep_d, 0, 1000.0, ids_d, table_d, leaf, sizes)
    assert rc == 0 and _guards_intact(bufs)
    _direct_equals(levels, labels, views, lv, sizes)


def test_equal_sizes_without_a_leaf_column_equal_ingest_frame():
    from hsr_utils import ingest_frame, ingest_frame_planes
    src, sizes = (37, 23), [(37, 23), (18, 11), (40, 30)]
    col, dep = I.make_frame(*src, seed=12)
    ids, table = _ids(src, seed=13), torch.from_numpy(_table(3, False)).cuda()
    for kw_old, kw_new in ((dict(), dict()), (dict(labels=ids), dict(labels=ids)),
                           (dict(labels=ids, tree_table=table), dict(labels=ids, label_table=table))):
        a, la = ingest_frame(col, dep, sizes, 6553.5, **kw_old)
        b, lb = ingest_frame_planes(col, dep, sizes, 6553.5, **kw_new)
        for (c0, d0), (c1, d1) in zip(a, b):
            assert torch.equal(c0.view(torch.int32), c1.view(torch.int32)) and torch.equal(d0.view(torch.int32), d1.view(torch.int32))
        assert (la is None and lb is None) or torch.equal(la, lb)
    _check(b, lb, *P.frame(col, dep, sizes, 6553.5, ids, table.cpu().numpy(), False))


def test_host_and_device_inputs_agree_and_one_library_call(monkeypatch):
    from hsr_utils import frames, ingest_frame_planes
    calls, old_calls = [], []
    real, real_old = frames._lib.hsr_frame_ingest_planes, frames._lib.hsr_frame_ingest
    monkeypatch.setattr(frames._lib, "hsr_frame_ingest_planes", lambda *a: calls.append(a) or real(*a))
    monkeypatch.setattr(frames._lib, "hsr_frame_ingest", lambda *a: old_calls.append(a) or real_old(*a))
    sizes = SHAPES["three-sizes"][3]
    col, dep, ids, table, (want_levels, want_labels) = _case("three-sizes")
    table_d = torch.from_numpy(table).cuda()
    a, la = ingest_frame_planes(col, dep, sizes, 1000.0, labels=ids.astype(np.int64), label_table=table_d, leaf_column=True)      # numpy
    assert len(calls) == 1 and old_calls == []                                                  # three levels and the labels: one call
    b, lb = ingest_frame_planes(torch.from_numpy(col), torch.from_numpy(dep.view(np.int16)), sizes, 1000.0, labels=torch.from_numpy(ids),
                                label_table=torch.from_numpy(table), leaf_column=True)                                          # host tensors
    wide = torch.zeros((7, 18, 3), dtype=torch.uint8, device="cuda")
    wide[:, ::2] = torch.from_numpy(col).cuda()
    c, lc = ingest_frame_planes(wide[:, ::2], torch.from_numpy(dep.view(np.int16)).cuda(), sizes, 1000.0, labels=torch.from_numpy(ids).cuda(),
                                label_table=table_d, leaf_column=True)                                                          # non-contiguous
    assert len(calls) == 3 and old_calls == []
    for levels, labels in ((a, la), (b, lb), (c, lc)):
        _check(levels, labels, want_levels, want_labels)
    for bad in ([], [(2, 3)] * 4, [(0, 3)]):      # the wrapper's refusals launch nothing
        with pytest.raises(ValueError, match="ingest_frame_planes"):
            ingest_frame_planes(col, dep, bad, 1000.0)
    assert len(calls) == 3


def test_refusals_set_the_error_and_write_nothing():
    """every refusal of the C entry, with device pointers in place: an error code, hsr_last_error() naming the entry and the argument,
    and the sentinel-filled outputs unchanged"""
    from diff_gaussian_rasterization import _abi
    sizes = [(4, 6), (2, 2), (3, 3)]
    col, dep, ids, table, _want = _case("three-sizes")
    col_d, dep_d, ids_d, table_d = (torch.from_numpy(col).cuda(), torch.from_numpy(dep.view(np.int16)).cuda(), torch.from_numpy(ids).cuda(),
                                    torch.from_numpy(table).cuda())
    for over, message in ((dict(Hc=0), b"sides"), (dict(Wc=16385), b"sides"), (dict(Hd=0), b"sides"), (dict(Wd=16385), b"sides"),
                          (dict(Hl=0), b"sides"), (dict(Wl=16385), b"sides"), (dict(level_sizes=[(4, 6), (2, 16385), (3, 3)]), b"sides"),
                          (dict(n_out=0), b"n_out"), (dict(n_out=4), b"n_out"), (dict(depth_type=3), b"depth_type"),
                          (dict(scale=0.0), b"depth_scale"), (dict(scale=float("nan")), b"depth_scale"),
                          (dict(L=17), b"num_levels"), (dict(L=-1), b"num_levels"), (dict(leaf=2), b"num_levels"), (dict(leaf=-1), b"num_levels"),
                          (dict(table=None), b"num_levels"), (dict(n_ids=0), b"num_levels"), (dict(L=0, leaf=1, table=None), b"num_levels")):
        rc, views, lv, bufs = _entry(col_d, dep_d, 0, 1000.0, ids_d, table_d, True, sizes, over)
        err = _abi.lib.hsr_last_error()
        assert rc == -1 and err.startswith(b"frame_ingest_planes: ") and message in err, (over, rc, err)
        assert all(bool((b == fill).all()) for b, fill in bufs), over
    # NULL pointers: labels without out_labels is one the helper cannot express; the colour image can
    from diff_gaussian_rasterization._abi import hsr_ingest_level
    out = torch.full((64,), FILL, device="cuda")
    arr = (hsr_ingest_level * 1)(hsr_ingest_level(2, 2, out.data_ptr(), out.data_ptr()))
    for color, labels, out_labels in ((None, None, None), (col_d.data_ptr(), ids_d.data_ptr(), None), (col_d.data_ptr(), None, out.data_ptr())):
        rc = _abi.lib.hsr_frame_ingest_planes(7, 9, color, 3, 5, dep_d.data_ptr(), 0, 1000.0, 11, 4, labels, 0, None, 0, 0, 1, arr, out_labels,
                                              torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == -1 and _abi.lib.hsr_last_error().startswith(b"frame_ingest_planes: NULL") and bool((out == FILL).all())
    rc, views, lv, bufs = _entry(col_d, dep_d, 0, 1000.0, ids_d, table_d, True, sizes)      # the same call with valid arguments does write
    assert rc == 0 and _guards_intact(bufs)
    assert not any(bool((v == FILL).any()) for pair in views for v in pair) and not bool((lv == LABEL_FILL).any())


def test_a_frame_of_scannets_size():
    """colour and labels 968x1296, depth 480x640, to the frame's 480x640 and a 240x320 level, with a 5-level + leaf table of 1358 rows"""
    from hsr_utils import ingest_frame_planes
    sizes = [(480, 640), (240, 320)]
    g = np.random.default_rng(21)
    smooth = np.add.outer(np.arange(968) * 3, np.arange(1296) * 2)[..., None] // 7 + np.array([0, 80, 160])
    col = ((smooth + g.integers(0, 24, size=smooth.shape)) % 256).astype(np.uint8)
    dep = g.integers(0, 8000, size=(480, 640)).astype(np.uint16)      # millimetres
    dep[100:140, 200:260] = 0
    ids = g.integers(0, 1400, size=(968, 1296)).astype(np.uint16)      # raw ids; those from 1358 on are beyond the table
    table = _table(5, True, seed=22, n_ids=1358)
    levels, labels = ingest_frame_planes(col, dep, sizes, 1000.0, labels=ids.astype(np.int32), label_table=torch.from_numpy(table).cuda(),
                                         leaf_column=True)
    want_levels, want = P.frame(col, dep, sizes, 1000.0, ids.astype(np.int32), table, True)
    assert want.shape == (6, 480, 640) and (want[5] >= 1358).any()
    _check(levels, labels, want_levels, want)
    assert np.array_equal(want_levels[0][1], (dep.astype(np.float64) / 1000.0).astype(np.float32))      # the depth at its own size
