"""CPU suite for the device export of the map as PLY records: the prototype of include/ext/hsr_map_export.h (its name and type classes;
tests/test_abi.py checks that it is exported and bound with the header's types), the job structure's layout, every refusal of the
header, the host-built colour table of the per-level export against a literal restatement of the reference's lines, and the numpy
restatement of the header (tests/map_export_ref.py) against the host writers hsr_utils.map_io.save_ply / save_ply_semantic, byte for
byte.  Nothing here launches: there is no GPU."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import map_export_ref as R
import test_abi

EXT_HEADER = "ext/hsr_map_export.h"
FIELDS = ["P", "S", "record", "colour", "means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales", "normals", "colours",
          "labels", "semantic", "table", "n", "K", "L", "sizes", "out", "out_labels"]
POINTERS = ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales", "normals", "colours", "labels", "semantic",
            "table", "out", "out_labels")


def test_map_export_abi_exported_and_bound():
    from diff_gaussian_rasterization import _abi
    protos = test_abi._prototypes([EXT_HEADER])
    assert [s[0] for s in _abi.HEADERS[EXT_HEADER]] == list(protos) == ["hsr_map_export"]
    assert protos["hsr_map_export"][2] == [("pointer", "hsr_map_export_job"), ("pointer", "void")]
    # the structure carries the field names of its typedef, in order, and the C layout
    structs = test_abi._structures([EXT_HEADER])
    job = _abi.hsr_map_export_job
    assert list(structs) == ["hsr_map_export_job"]
    assert structs["hsr_map_export_job"] == [f[0] for f in job._fields_] == FIELDS
    assert C.sizeof(job) == 192 and job.means3D.offset == 16 and job.table.offset == 88 and job.n.offset == 96
    assert job.sizes.offset == 108 and job.out.offset == 176 and job.out_labels.offset == 184
    from hsr_utils import evaluate, map_export
    defines = dict(re.findall(r"^#define\s+(HSR_\w+)\s+(\d+)\s*$", test_abi._source(EXT_HEADER), flags=re.M))
    assert map_export.MAP_EXPORT_MAX_P == int(defines["HSR_MAP_EXPORT_MAX_P"]) == (2 ** 31 - 1) // 68
    assert (map_export.RECORD_SH, map_export.RECORD_RGB8, map_export.RECORD_NONE) == tuple(
        int(defines["HSR_MAP_RECORD_" + k]) for k in ("SH", "RGB8", "NONE")) == (0, 1, 2)
    assert (map_export.COLOUR_GIVEN, map_export.COLOUR_LABELS, map_export.COLOUR_TREE) == tuple(
        int(defines["HSR_MAP_COLOUR_" + k]) for k in ("GIVEN", "LABELS", "TREE")) == (0, 1, 2)
    assert len(job().sizes) == evaluate.MAX_LEVELS and map_export.RECORD_BYTES == {0: R.SH_BYTES, 1: R.RGB8_BYTES}
    assert [tuple(f) for f in R.FIELDS_SH] == list(map_export.FIELDS_SH) and [tuple(f) for f in R.FIELDS_RGB8] == list(map_export.FIELDS_RGB8)


def test_names_are_reached_lazily_from_the_package():
    import hsr_utils
    from hsr_utils import map_export
    for name in ("export_map", "gaussian_tree_labels", "level_prefix_colour_table", "leaf_head_labels", "save_map_ply", "save_map_ply_semantic"):
        assert getattr(hsr_utils, name) is getattr(map_export, name)
    assert hasattr(hsr_utils.SlamSession, "export_map")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
# a valid job of each kind: every pointer non-NULL (dummies here, device memory in the GPU suite), P = 8
BASES = {
    "sh": dict(record=0),
    "given": dict(record=1, colour=0),
    "labels": dict(record=1, colour=1, n=256),
    "tree": dict(record=1, colour=2, L=3, sizes=(4, 8, 8), n=256, K=20),
    "none": dict(record=2, L=3, sizes=(4, 8, 8), K=20),
}
MAP_ARRAYS = ("means3D", "unnorm_rotations", "logit_opacities", "log_scales", "out")
MAX_P = (2 ** 31 - 1) // 68


def make_job(P=8, S=1, sizes=(), **kw):
    from diff_gaussian_rasterization import _abi
    fields = dict(P=P, S=S)
    fields.update({name: 4096 * (k + 1) for k, name in enumerate(POINTERS)})
    fields.update(kw)
    j = _abi.hsr_map_export_job(**fields)
    j.sizes[:len(sizes)] = list(sizes)
    return j


# every refusal the header lists, as (base, overrides of the job, a piece of the message); shared with the GPU suite, which runs them
# against canary-filled outputs
REFUSALS = (
    [(b, dict(P=p), b"P must be") for b in BASES for p in (-1, MAX_P + 1)]
    + [(b, dict(null_job=True), b"job is NULL") for b in ("sh", "none")]
    + [(b, dict(record=r), b"unknown record") for b in ("sh", "tree") for r in (3, -1)]
    + [(b, dict(S=s), b"S must be") for b in ("sh", "given", "labels", "tree") for s in (0, 2, 4, -1)]
    + [(b, {name: None}, b"NULL") for b in ("sh", "given", "labels", "tree") for name in MAP_ARRAYS]
    + [("sh", dict(rgb_colors=None), b"NULL")]
    + [("given", dict(colour=c), b"unknown colour") for c in (3, -1)]
    + [("given", dict(colours=None), b"NULL colours")]
    + [("labels", dict(labels=None), b"NULL labels or table"), ("labels", dict(table=None), b"NULL labels or table"),
       ("tree", dict(table=None), b"NULL labels or table")]
    + [(b, dict(n=n), b"rows") for b in ("labels", "tree") for n in (0, -5)]
    + [(b, dict(semantic=None), b"semantic") for b in ("tree", "none")]
    + [(b, dict(L=L, sizes=(2,) * 16, n=4, K=64), b"L must be") for b in ("tree", "none") for L in (0, 17, -1)]
    + [(b, dict(L=3, sizes=(2, s, 2), n=4, K=64), b"classes") for b in ("tree", "none") for s in (0, -2)]
    + [(b, dict(L=3, sizes=(3, 5, 8), n=120, K=15), b"columns") for b in ("tree", "none")]
    + [("tree", dict(L=3, sizes=(3, 5, 8), n=n, K=16), b"rows") for n in (119, 121)]
    + [("tree", dict(L=16, sizes=(4,) * 16, n=1, K=64), b"rows")]      # 4^16 = 2^32: as an int it would be 0
    + [("none", dict(out_labels=None), b"without out_labels")]
)


def refused_call(lib, base, overrides):
    """hsr_map_export with the job `base` (keyword arguments of make_job) overridden by `overrides`"""
    kw = dict(base)
    kw.update(overrides)
    null_job = kw.pop("null_job", False)
    job = make_job(**kw)
    return lib.hsr_map_export(None if null_job else C.byref(job), None)


@pytest.mark.parametrize("base,overrides,message", REFUSALS, ids=["%d-%s" % (i, r[0]) for i, r in enumerate(REFUSALS)])
def test_map_export_refuses_before_any_device_work(base, overrides, message):
    """no pointer here is a device pointer: every call is refused before the launch, with a message"""
    from diff_gaussian_rasterization import _abi
    rc = refused_call(_abi.lib, BASES[base], overrides)
    err = _abi.lib.hsr_last_error()
    assert rc == -1 and b"map_export" in err and message in err, (base, overrides, err)


def test_an_empty_map_succeeds_with_null_pointers():
    """P = 0 launches nothing, and the pointers of its empty arrays may be NULL; the checks of the scalars still hold"""
    from diff_gaussian_rasterization import _abi
    null = {name: None for name in POINTERS if name != "table"}
    for base in BASES.values():
        assert refused_call(_abi.lib, base, dict(null, P=0)) == 0
    assert refused_call(_abi.lib, BASES["sh"], dict(null, P=0, S=2)) == -1 and b"S must be" in _abi.lib.hsr_last_error()
    assert refused_call(_abi.lib, BASES["tree"], dict(null, P=0, n=255)) == -1 and b"rows" in _abi.lib.hsr_last_error()


def test_export_map_argument_errors():
    from hsr_utils import map_export as M
    m = {k: torch.from_numpy(v) for k, v in R.make_map(5, 1, 12, 0).items()}
    with pytest.raises(ValueError, match="colour must be one of"):
        M.export_map(m, colour="rgb")
    with pytest.raises(ValueError, match="return_labels"):
        M.export_map(m, return_labels=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.export_map(m)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.gaussian_tree_labels(m["semantic"], [4, 8, 20])
    with pytest.raises(ValueError, match="i_level must be"):
        M.level_prefix_colour_table({(0,): 0}, [4, 8, 20], 2, device="cpu")
    with pytest.raises(ValueError, match="writes a file"):
        M.save_map_ply("unused.ply", m, return_labels=True)


# ---- the per-level colour table ------------------------------------------------------------------------------------------------------
# tree_id_classes_map of a 3-level tree of sizes 3, 4, 2 (then the leaf count): per level the dict of the label tuples of its prefix;
# some tuples are named by no key, one key names a label outside its level
TREE_SIZES = [3, 4, 2, 17]
TREE_ID_CLASSES_MAP = [
    {(0,): "a", (2,): "c"},
    {(0, 0): "aa", (0, 3): "ad", (2, 1): "cb", (1, 2): "bc", (0, 4): "out of range"},
    {(0, 0, 0): 0, (0, 0, 1): 1, (0, 3, 1): 2, (2, 1, 0): 3, (1, 2, 1): 4, (2, 3, 0): 5, (1, 0, 0): 6},
]


@pytest.mark.parametrize("i_level", [0, 1, 2])
def test_level_prefix_colour_table_equals_transfer_eachlevel_1(i_level):
    from hsr_utils.export import label_colormap
    from hsr_utils.map_export import level_prefix_colour_table
    sizes = TREE_SIZES[:i_level + 1]
    mapping = TREE_ID_CLASSES_MAP[i_level]
    table = level_prefix_colour_table(mapping, TREE_SIZES, i_level, device="cpu")
    assert table.dtype == torch.uint8 and tuple(table.shape) == (int(np.prod(sizes)), 3)
    g = np.random.default_rng(3 + i_level)
    levels = np.stack([g.integers(0, s, size=200) for s in sizes]).astype(np.int64)
    every = np.array(np.meshgrid(*[np.arange(s) for s in sizes], indexing="ij")).reshape(len(sizes), -1)
    levels[:, :every.shape[1]] = every                               # every tuple at least once
    want = R.multilevel_colours_literal(torch.from_numpy(levels), mapping, lambda n: label_colormap(n, "cpu").numpy())
    got = R.X.levels(levels[:, None, :], sizes, table.numpy())[0]
    assert np.array_equal(got, want)
    black = ~want.any(axis=1)
    named = {k for k in mapping if all(0 <= v < s for v, s in zip(k, sizes))}
    # position 0 of the colour map is black as well: only the tuples of the later keys are told from the unnamed ones
    assert black.any() and int((~black[:every.shape[1]]).sum()) == len(named) - 1


def test_a_later_key_wins_and_tensor_keys_are_taken():
    from hsr_utils.export import label_colormap
    from hsr_utils.map_export import level_prefix_colour_table
    mapping = {(1, 2): "first", torch.tensor([0, 1]): "tensor key", (2, 0): "x", torch.tensor([1, 2]): "again"}
    table = level_prefix_colour_table(mapping, [3, 4, 9], 1, device="cpu").numpy().reshape(3, 4, 3)
    cmap = label_colormap(4, "cpu").numpy()
    assert table[1, 2].tolist() == cmap[3].tolist() and table[0, 1].tolist() == cmap[1].tolist() and table[2, 0].tolist() == cmap[2].tolist()


# ---- the restatement against the host writers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_normals", [False, True], ids=["zeros", "normals"])
@pytest.mark.parametrize("S", [1, 3])
def test_restatement_equals_the_host_writers_byte_for_byte(tmp_path, S, with_normals):
    from hsr_utils import map_io
    m = R.make_map(301, S, 12, 40 + S)
    finite = dict(m)
    finite["rgb_colors"] = np.where(np.isnan(m["rgb_colors"]), np.float32(0.5), m["rgb_colors"])      # a NaN's payload is not stated
    normals = m["normals"] if with_normals else None
    with np.errstate(invalid="ignore", over="ignore"):
        path = map_io.save_ply(str(tmp_path / "a.ply"), m["means3D"], m["log_scales"], m["unnorm_rotations"], finite["rgb_colors"],
                               m["logit_opacities"], normals)
    want = R.header(301, R.FIELDS_SH) + R.body_sh(finite, normals).tobytes()
    assert open(path, "rb").read() == want
    el = map_io.read_ply(path)
    assert el.dtype.itemsize == R.SH_BYTES and [n for n in el.dtype.names] == [n for _k, n in R.FIELDS_SH]
    # the semantic file: the colours of the tree tuples.  save_ply_semantic goes through float64 columns, which keep every float32 and
    # quieten a signalling NaN: the copied arrays carry quiet NaNs only here
    quiet = {k: v.copy() for k, v in m.items()}
    for k in ("means3D", "unnorm_rotations", "logit_opacities", "log_scales", "normals"):
        bits = quiet[k].view(np.uint32)
        bits[bits == 0x7f800001] = 0x7fc00001
    normals = quiet["normals"] if with_normals else None
    sizes = (4, 8)
    table = np.random.default_rng(9).integers(1, 256, size=(32, 3)).astype(np.uint8)
    labels = map_io.transfer_tree_label(quiet["semantic"], list(sizes) + [20])
    assert np.array_equal(labels, R.tree_labels(quiet["semantic"], sizes))
    colours = table[labels[0] * 8 + labels[1]]
    assert np.array_equal(colours, R.colours_tree(quiet["semantic"], sizes, table))
    path = map_io.save_ply_semantic(str(tmp_path / "b.ply"), quiet["means3D"], quiet["log_scales"], quiet["unnorm_rotations"], colours,
                                    quiet["logit_opacities"], normals)
    want = R.header(301, R.FIELDS_RGB8) + R.body_rgb8(quiet, colours, normals).tobytes()
    assert open(path, "rb").read() == want
    from hsr_utils.map_export import ply_header
    assert ply_header(301, R.FIELDS_RGB8) == R.header(301, R.FIELDS_RGB8) and ply_header(0, R.FIELDS_SH) == R.header(0, R.FIELDS_SH)


def test_f_dc_is_numpys_float32_expression():
    from hsr_utils import map_io
    v = R.rgb_values()
    with np.errstate(invalid="ignore", over="ignore"):
        host = (np.asarray(v, np.float32) - 0.5) / map_io.C0
    assert host.dtype == np.float32
    mine = R.f_dc(v)
    nan = np.isnan(host)
    assert np.array_equal(nan, np.isnan(mine)) and np.array_equal(host[~nan].view(np.uint32), mine[~nan].view(np.uint32))
    assert mine[1] == 0 and mine[2] == np.float32(0.5) / R.C0F and np.isinf(mine[8]) and mine[3] < 0 < mine[4]
