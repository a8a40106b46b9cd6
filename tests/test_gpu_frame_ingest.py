"""GPU suite for hsr_utils.frames.ingest_frame / hsr_frame_ingest (include/ext/hsr_frame_ingest.h): every output is compared BIT FOR BIT
with the numpy restatement of the header, tests/ingest_ref.py (which tests/test_frame_ingest_cpu.py shows to agree with two independent
float64 restatements to 1e-10 grey levels).  Colour and depth are compared as int32 words, labels as int64; the one exception is a
NaN depth (float32 input), which must be a NaN where the restatement has one — a NaN's payload after a division is not part of the rule."""
import functools

import numpy as np
import pytest
import torch

import ingest_ref as I
import resample_ref as R

pytestmark = pytest.mark.gpu

IDS = ["%dx%d-%dx%d" % (s + d) for s, d in R.SIZE_PAIRS]
SCALES = (6553.5, 1000.0, 1.0)
# the second and third level of the multi-level calls: one smaller, one larger than most sources, both odd
EXTRA = ((3, 5), (41, 29))


@functools.lru_cache(maxsize=None)
def _frame(src):
    col, dep = I.make_frame(*src, seed=100 * src[0] + src[1])
    return col, dep, torch.from_numpy(col).cuda(), torch.from_numpy(dep.view(np.int16)).cuda()


@functools.lru_cache(maxsize=None)
def _reference(src, dst, scale):
    col, dep, _c, _d = _frame(src)
    return I.color(col, dst), I.depth(dep, dst, scale)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_depth(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _check(got, want_color, want_depth):
    c, d = got
    assert c.dtype == d.dtype == torch.float32 and c.is_contiguous() and d.is_contiguous()
    assert tuple(c.shape) == want_color.shape and tuple(d.shape) == (1,) + want_depth.shape
    assert np.array_equal(_bits(c.cpu().numpy()), _bits(want_color))
    assert _same_depth(d.cpu().numpy()[0], want_depth)


@pytest.mark.parametrize("n_levels", [1, 2, 3])
@pytest.mark.parametrize("src,dst", R.SIZE_PAIRS, ids=IDS)
def test_levels_match_the_restatement_bit_for_bit(src, dst, n_levels):
    from hsr_utils import ingest_frame
    _col, _dep, col_d, dep_d = _frame(src)
    sizes = [dst] + list(EXTRA[:n_levels - 1])
    levels, labels = ingest_frame(col_d, dep_d, sizes, 6553.5)
    assert labels is None and len(levels) == n_levels
    for size, got in zip(sizes, levels):
        _check(got, *_reference(src, size, 6553.5))
    again, _ = ingest_frame(col_d, dep_d, sizes, 6553.5)      # two calls are bit-identical
    for a, b in zip(again, levels):
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_equal_sizes_give_every_grey_level_exactly():
    from hsr_utils import ingest_frame
    col = np.arange(16 * 16 * 3, dtype=np.int64).reshape(16, 16, 3)
    col = ((col // 3 + 85 * (col % 3)) % 256).astype(np.uint8)      # each channel holds all 256 grey levels
    assert all(len(np.unique(col[..., ch])) == 256 for ch in range(3))
    dep = np.arange(256, dtype=np.uint16).reshape(16, 16)
    (c, d), = ingest_frame(col, dep, [(16, 16)], 1.0)[0]
    want = col.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    assert np.array_equal(_bits(c.cpu().numpy()), _bits(want)) and np.array_equal(_bits(want), _bits(I.color(col, (16, 16))))
    assert float(c.min()) == 0.0 and float(c.max()) == 1.0
    assert np.array_equal(d.cpu().numpy()[0], dep.astype(np.float32))


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("kind", ["uint16", "int16-bits", "int32", "float32"])
def test_depth_types_and_scales(kind, scale):
    from hsr_utils import ingest_frame
    src, sizes = (37, 23), [(37, 23), (18, 11), (40, 30)]
    col, dep16, col_d, _d = _frame(src)
    if kind in ("uint16", "int16-bits"):
        raw = dep16.copy()
        raw[1, :4] = (0, 65535, 32768, 32767)      # the sign bit of the int16 view is part of the value
        given = raw if kind == "uint16" else torch.from_numpy(raw.view(np.int16))
    elif kind == "int32":
        raw = dep16.astype(np.int32) * 30000
        raw[1, :4] = (0, 2 ** 31 - 1, -5, 65536)
        given = torch.from_numpy(raw).cuda()
    else:
        raw = dep16.astype(np.float32) * np.float32(0.37)
        raw[1, :5] = (np.nan, np.inf, 0.0, -np.inf, 1e-30)
        raw[5:9, 3:9] = 0.0
        given = torch.from_numpy(raw)
    levels, _ = ingest_frame(col_d, given, sizes, scale)
    for size, (c, d) in zip(sizes, levels):
        want = I.depth(raw, size, scale)
        got = d.cpu().numpy()[0]
        assert _same_depth(got, want), (kind, scale, size)
        assert np.array_equal(_bits(c.cpu().numpy()), _bits(I.color(col, size)))
    full = levels[0][1].cpu().numpy()[0]
    if kind == "float32":
        assert np.isnan(full[1, 0]) and full[1, 1] == np.inf and full[1, 2] == 0.0 and full[1, 3] == -np.inf and not full[5:9, 3:9].any()
    elif kind != "int32":
        assert full[1, 0] == 0.0 and full[1, 1] == np.float32(65535.0 / scale) and full[1, 2] == np.float32(32768.0 / scale)


def _label_case(L, seed=5):
    """(ids int32 [33,65] with negative ids and ids beyond the table, table int32 [12,L] with -1 entries | None)"""
    g = np.random.default_rng(seed)
    ids = g.integers(-2, 16, size=(33, 65)).astype(np.int32)      # the table knows 0..11
    ids[0, :3] = (-2147483648, 2147483647, 11)
    if L == 0:
        return ids, None
    table = g.integers(-1, 40, size=(12, L)).astype(np.int32)
    table[3] = -1
    return ids, table


@pytest.mark.parametrize("dtype", [np.int32, np.int64, np.uint8], ids=["int32", "int64", "uint8"])
@pytest.mark.parametrize("L", [0, 1, 3, 5])
def test_labels_at_a_reduced_level_0(L, dtype):
    from hsr_utils import ingest_frame
    src, sizes = (33, 65), [(17, 33), (33, 65)]      # level 0 is the reduced one; the labels follow it
    col, dep, col_d, dep_d = _frame(src)
    ids, table = _label_case(L)
    if dtype is np.uint8:
        ids = (ids & 15).astype(np.int32)
    elif dtype is np.int64:
        ids[0, :2] = (-7, 100000)      # int64 ids travel as int32
    given = ids.astype(dtype)
    table_d = None if table is None else torch.from_numpy(table).cuda()
    levels, labels = ingest_frame(col_d, dep_d, sizes, 1000.0, labels=given, tree_table=table_d)
    want = I.labels(ids, sizes[0], table)
    assert labels.dtype == torch.int64 and labels.is_contiguous() and tuple(labels.shape) == (L + 1,) + sizes[0] == want.shape
    assert np.array_equal(labels.cpu().numpy(), want)
    for size, got in zip(sizes, levels):
        _check(got, *_reference(src, size, 1000.0))
    if L and dtype is np.int32:
        unknown = (want[L] < 0) | (want[L] >= 12)
        assert unknown.any() and all(np.array_equal(want[l][unknown], want[L][unknown]) for l in range(L))      # the raw id on every level
        assert (want[:L][:, want[L] == 3] == -1).all() and (want[L] == 3).any()


@pytest.mark.parametrize("src", [(97, 130), (37, 23)], ids=["97x130", "37x23"])
def test_three_levels_equal_three_one_level_calls(src):
    from hsr_utils import ingest_frame
    _col, _dep, col_d, dep_d = _frame(src)
    ids = torch.from_numpy(np.random.default_rng(9).integers(0, 12, size=src).astype(np.int32)).cuda()
    table = torch.from_numpy(_label_case(3)[1]).cuda()
    sizes = [(48, 64), (18, 11), (97, 130)]
    levels, labels = ingest_frame(col_d, dep_d, sizes, 6553.5, labels=ids, tree_table=table)
    for k, size in enumerate(sizes):
        one, one_labels = ingest_frame(col_d, dep_d, [size], 6553.5, labels=ids, tree_table=table)
        assert torch.equal(one[0][0].view(torch.int32), levels[k][0].view(torch.int32))
        assert torch.equal(one[0][1].view(torch.int32), levels[k][1].view(torch.int32))
        if k == 0:
            assert torch.equal(one_labels, labels)


def test_host_and_device_inputs_agree():
    from hsr_utils import ingest_frame
    src, sizes = (33, 65), [(17, 33), (40, 70)]
    col, dep, col_d, dep_d = _frame(src)
    ids, table = _label_case(3)
    table_d = torch.from_numpy(table).cuda()
    a, la = ingest_frame(col, dep, sizes, 1000.0, labels=ids, tree_table=table_d)                                # numpy
    b, lb = ingest_frame(torch.from_numpy(col), torch.from_numpy(dep.view(np.int16)), sizes, 1000.0, labels=torch.from_numpy(ids),
                         tree_table=torch.from_numpy(table))                                                      # host tensors
    wide = torch.zeros((33, 130, 3), dtype=torch.uint8, device="cuda")
    wide[:, ::2] = col_d
    c, lc = ingest_frame(wide[:, ::2], dep_d, sizes, 1000.0, labels=torch.from_numpy(ids).cuda(), tree_table=table_d)      # non-contiguous
    assert not wide[:, ::2].is_contiguous()
    for other, lo in ((b, lb), (c, lc)):
        assert torch.equal(la, lo)
        for (c0, d0), (c1, d1) in zip(a, other):
            assert torch.equal(c0.view(torch.int32), c1.view(torch.int32)) and torch.equal(d0.view(torch.int32), d1.view(torch.int32))
    for size, got in zip(sizes, a):
        _check(got, *_reference(src, size, 1000.0))


def test_invalid_arguments_write_nothing():
    """the C entry point itself: a side of 16385 (no allocation of that size), n_out = 4, L > 0 without a table, scale 0 — each an
    error code, and the sentinel-filled outputs unchanged"""
    from diff_gaussian_rasterization import _abi
    src, dst = (5, 7), (4, 6)
    _col, _dep, col_d, dep_d = _frame(src)
    ids = torch.zeros(src, dtype=torch.int32, device="cuda")
    table = torch.zeros((4, 2), dtype=torch.int32, device="cuda")
    fill = -7.25
    out_c = [torch.full((3 * 24,), fill, device="cuda") for _ in range(4)]
    out_d = [torch.full((24,), fill, device="cuda") for _ in range(4)]
    out_l = torch.full((3 * 24,), -99, dtype=torch.int64, device="cuda")

    def call(Hs=src[0], Ws=src[1], scale=1000.0, L=2, tab=table, n_ids=4, n_out=1, sizes=(dst,) * 4):
        arr = (_abi.hsr_ingest_level * 4)(*[_abi.hsr_ingest_level(h, w, c.data_ptr(), d.data_ptr()) for (h, w), c, d in zip(sizes, out_c, out_d)])
        with torch.cuda.device(col_d.device):
            rc = _abi.lib.hsr_frame_ingest(Hs, Ws, col_d.data_ptr(), dep_d.data_ptr(), 0, scale, ids.data_ptr(), L,
                                           None if tab is None else tab.data_ptr(), n_ids, n_out, arr, out_l.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, _abi.lib.hsr_last_error()
    for kw, message in ((dict(Ws=16385), b"sides"), (dict(sizes=((4, 16385),) + (dst,) * 3), b"sides"), (dict(n_out=4), b"n_out"),
                        (dict(tab=None), b"num_levels"), (dict(scale=0.0), b"depth_scale")):
        rc, err = call(**kw)
        assert rc == -1 and message in err, (kw, rc, err)
        assert all(bool((t == fill).all()) for t in out_c + out_d) and bool((out_l == -99).all()), kw
    rc, _err = call()      # the same call with valid arguments does write: level 0 alone
    assert rc == 0
    assert not bool((out_c[0] == fill).any()) and not bool((out_d[0] == fill).any()) and not bool((out_l == -99).any())
    assert all(bool((t == fill).all()) for t in out_c[1:] + out_d[1:])


def test_wrapper_refusals_launch_nothing(monkeypatch):
    from hsr_utils import frames, ingest_frame
    calls = []
    real = frames._lib.hsr_frame_ingest
    monkeypatch.setattr(frames._lib, "hsr_frame_ingest", lambda *a: calls.append(a) or real(*a))
    col, dep, col_d, dep_d = _frame((5, 7))
    for bad in ([], [(2, 3)] * 4, [(0, 3)], [(2, 16385)]):
        with pytest.raises(ValueError, match="ingest_frame"):
            ingest_frame(col_d, dep_d, bad, 1000.0)
    with pytest.raises(ValueError, match="png_depth_scale"):
        ingest_frame(col_d, dep_d, [(2, 3)], 0.0)
    with pytest.raises(RuntimeError, match="color_u8 must be"):
        ingest_frame(col_d.permute(2, 0, 1), dep_d, [(2, 3)], 1000.0)
    with pytest.raises(RuntimeError, match="depth_raw must be"):
        ingest_frame(col_d, dep_d.double(), [(2, 3)], 1000.0)
    assert calls == []
    ingest_frame(col_d, dep_d, [(2, 3), (5, 7), (9, 9)], 1000.0)
    assert len(calls) == 1      # three levels, one launch
