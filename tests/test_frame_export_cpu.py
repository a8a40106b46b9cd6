"""CPU suite for the export of an evaluated frame's pictures: the prototype of include/ext/hsr_frame_export.h (its name, type classes
and job structure; tests/test_abi.py checks that it is exported and bound with the header's types), its argument checks, the three host-built
colour tables of hsr_utils.export, and the numpy restatement of the header (tests/export_ref.py) against a literal restatement of the
reference's lines.  Nothing here launches: there is no GPU."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import export_ref as X
import test_abi

EXT_HEADER = "ext/hsr_frame_export.h"


def test_frame_export_abi_exported_and_bound():
    from diff_gaussian_rasterization import _abi
    protos = test_abi._prototypes([EXT_HEADER])
    assert [s[0] for s in _abi.HEADERS[EXT_HEADER]] == list(protos) == ["hsr_frame_export"]
    assert protos["hsr_frame_export"][2] == ["int", "int", "int", ("pointer", "hsr_export_job"), ("pointer", "void")]
    # the structure carries the field names of its typedef, in order, and the C layout
    structs = test_abi._structures([EXT_HEADER])
    assert list(structs) == ["hsr_export_job"]
    assert structs["hsr_export_job"] == [f[0] for f in _abi.hsr_export_job._fields_] == ["kind", "src", "table", "n", "K", "L", "sizes", "lo",
                                                                                         "hi", "out"]
    assert C.sizeof(_abi.hsr_export_job) == 120 and _abi.hsr_export_job.sizes.offset == 36 and _abi.hsr_export_job.out.offset == 112
    from hsr_utils import evaluate, export, slam
    defines = dict(re.findall(r"^#define\s+(HSR_\w+)\s+(\d+)\s*$", test_abi._source(EXT_HEADER), flags=re.M))
    assert export.EXPORT_MAX_JOBS == int(defines["HSR_EXPORT_MAX_JOBS"]) == 8 == len(export.PICTURES)
    assert (export.COLOR, export.DEPTH, export.LABELS, export.LEVELS, export.LOGITS) == tuple(
        int(defines["HSR_EXPORT_" + k]) for k in ("COLOR", "DEPTH", "LABELS", "LEVELS", "LOGITS")) == (0, 1, 2, 3, 4)
    assert export.EXPORT_MAX_SIDE == slam.RESAMPLE_MAX_SIDE and len(_abi.hsr_export_job().sizes) == evaluate.MAX_LEVELS


def _job(kind, src=4096, table=8192, n=256, K=0, L=0, sizes=(), lo=0.0, hi=6.0, out=12288):
    from diff_gaussian_rasterization import _abi
    j = _abi.hsr_export_job(kind=kind, src=src, table=table, n=n, K=K, L=L, lo=lo, hi=hi, out=out)
    j.sizes[:len(sizes)] = list(sizes)
    return j


# every refusal the header lists, as (keyword arguments of the call, a piece of the message); shared with the GPU suite, which runs them
# against canary-filled outputs
REFUSALS = (
    [(dict(H=h), b"sides") for h in (0, -1, 16385)] + [(dict(W=w), b"sides") for w in (0, 16385)]
    + [(dict(n_jobs=n), b"n_jobs") for n in (0, 9, -1)] + [(dict(null_jobs=True), b"n_jobs")]
    + [(dict(job=dict(kind=k)), b"unknown kind") for k in (5, -1)]
    + [(dict(job=dict(kind=k, src=None)), b"NULL") for k in range(5)] + [(dict(job=dict(kind=k, out=None)), b"NULL") for k in range(5)]
    + [(dict(job=dict(kind=k, table=None)), b"NULL") for k in (1, 2, 3, 4)]
    + [(dict(job=dict(kind=1, lo=lo, hi=hi)), b"hi - lo") for lo, hi in ((0.0, 0.0), (6.0, 0.0), (0.0, float("inf")), (0.0, float("nan")),
                                                                          (float("-inf"), 0.0), (-3e38, 3e38))]
    + [(dict(job=dict(kind=1, n=255)), b"rows"), (dict(job=dict(kind=2, n=0)), b"rows")]
    + [(dict(job=dict(kind=k, L=L, sizes=(2,) * 16, n=4, K=64)), b"L must be") for k in (3, 4) for L in (0, 17, -1)]
    + [(dict(job=dict(kind=k, L=3, sizes=(2, s, 2), n=4, K=64)), b"classes") for k in (3, 4) for s in (0, -2)]
    + [(dict(job=dict(kind=4, L=3, sizes=(3, 5, 8), n=120, K=15)), b"planes")]
    + [(dict(job=dict(kind=k, L=3, sizes=(3, 5, 8), n=n, K=16)), b"rows") for k in (3, 4) for n in (119, 121, 0)]
    + [(dict(job=dict(kind=3, L=16, sizes=(4,) * 16, n=0)), b"rows")]      # 4^16 = 2^32: as an int it would be 0
    + [(dict(n_jobs=2, second=dict(kind=2, n=0)), b"job 1")]                # the later job of two
)


def refused_call(lib, base, H=8, W=8, n_jobs=1, null_jobs=False, job=None, second=None):
    """hsr_frame_export with job 0 = `base` overridden by `job` (and, for n_jobs = 2, job 1 by `second`)"""
    from diff_gaussian_rasterization import _abi
    arr = (_abi.hsr_export_job * 9)()
    for k in range(9):
        kw = dict(base)
        kw.update((job if k == 0 else second if k == 1 else None) or {})
        arr[k] = _job(**kw)
    return lib.hsr_frame_export(H, W, n_jobs, None if null_jobs else arr, None)


@pytest.mark.parametrize("kw,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_frame_export_refuses_before_any_device_work(kw, message):
    """no pointer here is a device pointer: every call is refused before the launch, with a message"""
    from diff_gaussian_rasterization import _abi
    rc = refused_call(_abi.lib, dict(kind=0), **kw)
    assert rc == -1 and b"frame_export" in _abi.lib.hsr_last_error() and message in _abi.lib.hsr_last_error(), (kw, _abi.lib.hsr_last_error())


def test_jet_colormap():
    from hsr_utils.export import jet_colormap
    t = jet_colormap("cpu")
    assert t.dtype == torch.uint8 and tuple(t.shape) == (256, 3)
    j = t.numpy().astype(np.int64)
    assert j[0].tolist() == [0, 0, 128] and j[255].tolist() == [128, 0, 0] and j[96].tolist() == [2, 255, 254]
    assert j[32].tolist() == [0, 1, 255] and j[159].tolist() == [254, 255, 2]
    r, g, b = j[:, 0], j[:, 1], j[:, 2]
    assert np.array_equal(r, b[::-1]) and np.array_equal(g, g[::-1])
    # the closed form with halves rounded up, in exact rational arithmetic: 255 * clamp(1.5 - |4 i / 255 - c|, 0, 1) = T / 2
    from fractions import Fraction
    for i in range(256):
        for ch, c in enumerate((3, 2, 1)):
            v = 255 * min(max(Fraction(3, 2) - abs(Fraction(4 * i, 255) - c), 0), 1)
            assert j[i, ch] == (2 * v + 1) // 2, (i, ch)
    # piecewise monotone: up, flat at 255, down (each channel one trapezoid, blue and red cut off by the table's ends)
    for ch in (r, g, b):
        d = np.sign(np.diff(ch))
        d = d[d != 0]
        assert (np.diff(d) <= 0).all() and ch.max() == 255      # rises come before falls


def test_label_colormap():
    from hsr_utils.export import label_colormap
    t = label_colormap(256, "cpu")
    assert t.dtype == torch.uint8 and tuple(t.shape) == (256, 3)
    assert t[:4].tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0]] and t[8].tolist() == [64, 0, 0]
    assert t[7].tolist() == [128, 128, 128] and t[255].tolist() == [224, 224, 192] and t[64].tolist() == [32, 0, 0]
    assert len({tuple(row) for row in t.tolist()}) == 256 and torch.equal(label_colormap(9, "cpu"), t[:9])
    with pytest.raises(ValueError, match="n >= 1"):
        label_colormap(0, "cpu")


# the colours of a 3-level tree of sizes 3, 4, 2: duplicate matches (a later key wins; the tensor key repeats the tuple before it, as the
# reference's tensor keys can), -1 keys, tuples no key names
COLOUR_MAP = {(0, 0, 0): (10, 20, 30), (0, -1, -1): (40, 50, 60), (1, 2, -1): (70, 80, 90), (1, 2, 1): (100, 110, 120), (2, 3, 1): (1, 2, 3),
              (-1, 1, 0): (200, 210, 220), torch.tensor([2, 3, 1]): (4, 5, 6), (0, 1, 1): (130, 140, 150), (1, -1, 0): (160, 170, 180), (2, 0, 0): (9, 9, 9)}
TREE_SIZES = [3, 4, 2, 17]      # the levels, then the leaf count (not read)


@pytest.mark.parametrize("wildcard", [True, False], ids=["replica", "scannet"])
def test_tuple_colour_table_equals_the_per_key_masks(wildcard):
    from hsr_utils.export import tuple_colour_table
    table = tuple_colour_table(COLOUR_MAP, TREE_SIZES, wildcard, device="cpu")
    assert table.dtype == torch.uint8 and tuple(table.shape) == (24, 3)
    g = np.random.default_rng(11)
    planes = np.stack([g.integers(0, s, size=(29, 31)) for s in TREE_SIZES[:-1]]).astype(np.int64)
    planes[:, 0, :24] = np.array([[a, b, c] for a in range(3) for b in range(4) for c in range(2)]).T      # every tuple at least once
    want = (X.vis_replica if wildcard else X.vis_scannet)(torch.from_numpy(planes), COLOUR_MAP)
    got = X.levels(planes, TREE_SIZES[:-1], table.numpy())
    assert np.array_equal(got, want)
    t = table.numpy().reshape(3, 4, 2, 3)
    assert t[2, 3, 1].tolist() == [4, 5, 6]                      # the later of two equal keys
    assert t[2, 1, 1].tolist() == [0, 0, 0]                      # a tuple no key names
    assert t[2, 0, 0].tolist() == [9, 9, 9]
    if wildcard:
        assert t[0, 0, 0].tolist() == [40, 50, 60] and t[0, 1, 1].tolist() == [130, 140, 150] and t[0, 1, 0].tolist() == [200, 210, 220]
        assert t[1, 2, 1].tolist() == [100, 110, 120] and t[1, 2, 0].tolist() == [160, 170, 180] and t[1, 1, 0].tolist() == [160, 170, 180]
    else:
        assert t[0, 0, 0].tolist() == [10, 20, 30] and t[0, 1, 0].tolist() == [0, 0, 0] and t[1, 2, 0].tolist() == [0, 0, 0]
        assert int((t.reshape(24, 3).any(axis=1)).sum()) == 5   # the five keys without a -1


def test_tuple_colour_table_edges():
    from hsr_utils.export import tuple_colour_table
    every = tuple_colour_table({(-1, -1): (7, 8, 9), (1, 5): (1, 1, 1), (3, 0): (2, 2, 2)}, [2, 3, 6], True, device="cpu")
    assert every.tolist() == [[7, 8, 9]] * 6                     # a key of -1 alone matches every tuple; out-of-range keys match nothing
    assert tuple_colour_table({(-1, -1): (7, 8, 9)}, [2, 3, 6], False, device="cpu").tolist() == [[0, 0, 0]] * 6
    keys = tuple_colour_table({torch.tensor([1, 0]): np.array([3, 4, 5], dtype=np.uint8)}, [2, 3, 6], True, device="cpu")
    assert keys[3].tolist() == [3, 4, 5] and int(keys.sum()) == 12
    with pytest.raises(RuntimeError, match="has 3 levels"):
        tuple_colour_table({(0, 0, 0): (1, 1, 1)}, [2, 3, 6], True, device="cpu")
    with pytest.raises(RuntimeError, match="0..255"):
        tuple_colour_table({(0, 0): (1, 1, 256)}, [2, 3, 6], True, device="cpu")
    with pytest.raises(RuntimeError, match="too large"):
        tuple_colour_table({}, [1 << 13, 1 << 13, 2, 5], True, device="cpu")
    with pytest.raises(RuntimeError, match="level sizes"):
        tuple_colour_table({}, [5], True, device="cpu")


def test_colour_ties_are_real_and_both_restatements_agree():
    v = X.colour_values()
    assert v.dtype == np.float32
    products = v[:255] * np.float32(255)
    assert products.dtype == np.float32 and np.array_equal(products.astype(np.float64), np.arange(255) + 0.5)      # all 255 are exact ties
    x = X.lay(v, (3, 1, len(v)))
    got, literal = X.color(x), X.color_literal(x)
    assert got.dtype == literal.dtype == np.uint8 and got.shape == literal.shape == (1, len(v), 3)
    assert np.array_equal(got, literal)
    k = np.arange(255)
    assert np.array_equal(got[0, :255, 0], k + (k % 2))           # halves to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, ..., 254.5 -> 254
    assert got[0, 255:264, 0].tolist() == [0, 255, 255, 0, 0, 0, 255, 0, 0]      # -1, 2, inf, -inf, NaN, 0, 1, -0, 1e-40
    assert got[0, 265:, 0].tolist() == [64, 128, 191, 255]        # 63.75, 127.5 (to even), 191.25, above 1


def test_depth_both_restatements_agree():
    from hsr_utils.export import jet_colormap
    table = jet_colormap("cpu").numpy()
    v = X.depth_values()
    d = X.lay(v, (2, len(v)), shift=3)
    got, literal = X.depth(d, table), X.depth_literal(d, table)
    assert got.dtype == np.uint8 and got.shape == (2, len(v), 3) and np.array_equal(got, literal)
    idx = np.arange(256)[:, None] * np.ones(3, dtype=np.int64)      # a table that shows the index itself
    shown = X.depth(v[None], idx.astype(np.uint8))[0, :, 0]
    assert shown[:10].tolist() == [0, 255, 255, 0, 0, 255, 0, 254, 0, 127]      # 0, 6, 7, -1, NaN, inf, -inf, just under 6, 1e-40, 3
    steps = shown[10:].astype(np.int64)
    # float32(6 k / 255) / 6 * 255 is k or just under it: the index is k or k - 1, never more, and both occur
    assert ((steps == np.arange(256)) | (steps == np.arange(256) - 1)).all() and (steps == np.arange(256)).any() and (steps != np.arange(256)).any()
    other = X.depth(d, table, lo=1.0, hi=3.5)
    with np.errstate(invalid="ignore"):
        n = (d - np.float32(1.0)) / np.float32(2.5)
    assert np.array_equal(other, table[(np.nan_to_num(np.clip(n, 0, 1), nan=0.0) * np.float32(255)).astype(np.uint8)])


def test_label_and_level_restatements():
    table = np.arange(15, dtype=np.uint8).reshape(5, 3) + 1
    lab = np.array([[0, 4, 5, -1, 2 ** 31 - 1, -2 ** 31]], dtype=np.int32)
    assert X.labels(lab, table)[0].tolist() == [[1, 2, 3], [13, 14, 15], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]      # no wrap of -1
    t6 = np.arange(18, dtype=np.uint8).reshape(6, 3) + 1
    lev = np.array([[[0, 1, 1, 2, -1, 0, 1 << 40, 0]], [[0, 0, 2, 0, 0, 3, 0, -(1 << 40)]]], dtype=np.int64)
    got = X.levels(lev, (2, 3), t6)[0]
    assert got[:3].tolist() == [[1, 2, 3], [10, 11, 12], [16, 17, 18]] and not got[3:].any()      # (0,0) -> 0, (1,0) -> 3, (1,2) -> 5
    x = np.zeros((6, 1, 3), dtype=np.float32)
    x[:, 0, 0] = (0.0, 1.0, 2.0, 2.0, 1.0, np.nan)      # level 0 (2 planes): plane 1; level 1 (3 planes): a tie, the first wins
    x[:, 0, 1] = 0.5                                      # all equal: index 0 on both levels
    x[:, 0, 2] = (3.0, -1.0, 0.0, 0.25, 0.25, np.nan)
    assert X.level_labels(x, (2, 3))[:, 0].tolist() == [[1, 0, 0], [0, 0, 1]]
    assert np.array_equal(X.logits(x, (2, 3), t6), X.levels(X.level_labels(x, (2, 3)), (2, 3), t6))


def test_export_frame_argument_errors():
    from hsr_utils.export import export_frame, write_png
    with pytest.raises(RuntimeError, match="at least one picture"):
        export_frame()
    with pytest.raises(RuntimeError, match="no CPU path"):
        export_frame(im=torch.zeros(3, 4, 6))
    with pytest.raises(RuntimeError, match="level_sizes and tuple_table"):
        export_frame(gt_levels=torch.zeros(2, 4, 6, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="label_table"):
        export_frame(labels=torch.zeros(4, 6, dtype=torch.int32))
    with pytest.raises(ValueError, match="depth_range"):
        export_frame(depth=torch.zeros(1, 4, 6), depth_range=(6.0, 6.0))
    with pytest.raises(RuntimeError, match="uint8"):
        write_png("unused.png", np.zeros((4, 6, 3), dtype=np.float32))


def test_write_png_round_trip(tmp_path):
    from PIL import Image
    from hsr_utils.export import write_png
    a = np.random.default_rng(2).integers(0, 256, size=(7, 5, 3)).astype(np.uint8)
    write_png(str(tmp_path / "a.png"), torch.from_numpy(a))
    write_png(str(tmp_path / "b.png"), a)
    for name in ("a.png", "b.png"):
        with Image.open(tmp_path / name) as im:
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), a)      # R, G, B as stored
