"""CPU suite for the ScanNet ingest: the prototype of include/ext/hsr_frame_ingest_planes.h (its name and type classes;
tests/test_abi.py checks that it is exported and bound with the header's types), the entry's refusals, composed_label_table against a literal
restatement of the reference's loops of masked assignments (tests/ingest_planes_ref.py), the two tsv readers and ScanNetSequence on
files the tests write, the argument errors of ingest_frame_planes, and the routing of SlamSession.ingest between the two ingest
functions.  Nothing here launches: there is no GPU."""
import inspect
import os

import numpy as np
import pytest
import torch

import ingest_planes_ref as P
import ingest_ref as I
import test_abi

EXT_HEADER = "ext/hsr_frame_ingest_planes.h"
NAME = "hsr_frame_ingest_planes"


def test_frame_ingest_planes_abi_exported_and_bound():
    from diff_gaussian_rasterization import _abi
    protos = test_abi._prototypes([EXT_HEADER])
    assert [s[0] for s in _abi.HEADERS[EXT_HEADER]] == list(protos) == [NAME]
    params = protos[NAME][2]
    assert len(params) == 19 and params[7] == "double" and params[16] == ("pointer", "hsr_ingest_level") and params[14] == "int"
    # the header reuses the structure and the defines of hsr_frame_ingest.h and declares none of its own
    src = test_abi._source(EXT_HEADER)
    assert '#include "hsr_frame_ingest.h"' in src and "typedef" not in src and "#define HSR_INGEST" not in src


def test_frame_ingest_planes_refuses_before_any_device_work():
    """bad sizes, counts, scales, tables and NULL pointers are an error code and a message, not a launch (no pointer here is a device
    pointer); the same call through hsr_frame_ingest names that entry"""
    from diff_gaussian_rasterization import _abi
    lib = _abi.lib
    fake = 4096      # never dereferenced: every call below is refused before the launch

    def call(Hc=8, Wc=8, color=fake, Hd=5, Wd=7, depth=fake, depth_type=0, scale=1000.0, Hl=3, Wl=9, labels=None, L=0, table=None, n_ids=0,
             leaf=0, n_out=1, sizes=((4, 4),), outs=(fake, fake), out_labels=None, levels="array"):
        arr = (_abi.hsr_ingest_level * 4)(*[_abi.hsr_ingest_level(h, w, outs[0], outs[1]) for h, w in (tuple(sizes) + ((4, 4),) * 4)[:4]])
        return lib.hsr_frame_ingest_planes(Hc, Wc, color, Hd, Wd, depth, depth_type, scale, Hl, Wl, labels, L, table, n_ids, leaf, n_out,
                                           arr if levels == "array" else None, out_labels, None)
    with_labels = dict(labels=fake, out_labels=fake)
    for kw in (dict(Hc=0), dict(Wc=16385), dict(Hd=0), dict(Hd=16385), dict(Wd=-1), dict(Wd=16385), dict(sizes=((0, 4),)),
               dict(n_out=3, sizes=((4, 4), (4, 4), (4, 16385))), dict(Hl=0, **with_labels), dict(Wl=16385, **with_labels),
               dict(Hl=-3, Wl=4, **with_labels)):
        assert call(**kw) == -1 and b"frame_ingest_planes: sides" in lib.hsr_last_error(), kw
    for kw in (dict(n_out=0), dict(n_out=4), dict(levels=None)):
        assert call(**kw) == -1 and b"frame_ingest_planes: n_out" in lib.hsr_last_error(), kw
    for kw in (dict(depth_type=3), dict(depth_type=-1)):
        assert call(**kw) == -1 and b"frame_ingest_planes: depth_type" in lib.hsr_last_error(), kw
    for kw in (dict(scale=0.0), dict(scale=float("inf")), dict(scale=float("nan"))):
        assert call(**kw) == -1 and b"frame_ingest_planes: depth_scale" in lib.hsr_last_error(), kw
    for kw in (dict(L=-1), dict(L=17, table=fake, n_ids=4), dict(L=2, **with_labels), dict(L=2, table=fake, n_ids=0, **with_labels),
               dict(leaf=2, table=fake, n_ids=4), dict(leaf=-1, table=fake, n_ids=4), dict(leaf=1, **with_labels),
               dict(leaf=1, table=fake, n_ids=0, **with_labels), dict(leaf=1, L=3, n_ids=5, **with_labels)):
        assert call(**kw) == -1 and b"frame_ingest_planes: num_levels" in lib.hsr_last_error(), kw
    # the label sides are not looked at without labels; what refuses these calls is the NULL colour image
    for kw in (dict(color=None), dict(depth=None), dict(outs=(None, fake)), dict(outs=(fake, None)), dict(labels=fake), dict(out_labels=fake),
               dict(color=None, Hl=0, Wl=0), dict(color=None, Hl=16385, Wl=-1), dict(color=None, leaf=1, table=fake, n_ids=1)):
        assert call(**kw) == -1 and b"frame_ingest_planes: NULL" in lib.hsr_last_error(), kw


# ---- composed_label_table -----------------------------------------------------------------------------------------------------------------
CLASSES = {1: 3, 2: 5, "3": 9, 4: 4, 7: 40, 12: 1, 13: 0}      # 3 is a key and the value of key 1: no chaining (1 -> 3, not 1 -> 9)
TREE4 = {0: (0, 0, 0, -1), 1: (1, 0, 2, 3), "3": (1, 1, 0, 0), 4: (2, 0, -1, -1), 5: (2, 1, 1, 7), 11: (3, 3, 3, 3), 40: (4, 0, 0, 0)}      # no 9


def _id_images(n_ids, seed):
    g = np.random.default_rng(seed)
    raw = g.integers(-3, n_ids + 6, size=(4, 23, 31)).astype(np.int64)      # ids below 0 and beyond the table among them
    raw[0, 0, :8] = (-1, n_ids, n_ids + 100000, 0, 3, 1, 7, 13)
    return raw


def _lookup(raw, table, leaf_column=True):
    return P.labels(raw, raw.shape, table.numpy(), leaf_column)


def test_composed_label_table_equals_the_reference_loops():
    from hsr_utils import composed_label_table
    from hsr_utils.frames import composed_label_table as from_frames
    assert composed_label_table is from_frames
    table = composed_label_table(CLASSES, TREE4, 4, device="cpu")
    assert table.dtype == torch.int32 and tuple(table.shape) == (41, 5)      # the largest key of either dict (tree: 40) + 1
    assert table[1].tolist() == [1, 1, 0, 0, 3]            # 1 -> 3 -> the tree's row of 3; NOT chained on to 9
    assert table[3].tolist() == [9, 9, 9, 9, 9]            # 3 -> 9, which the tree does not name: the leaf in every column
    assert table[6].tolist() == [6, 6, 6, 6, 6]            # in neither dict
    assert table[11].tolist() == [3, 3, 3, 3, 11]          # not in the class mapping, named by the tree
    assert table[7].tolist() == [4, 0, 0, 0, 40] and table[13].tolist() == [0, 0, 0, -1, 0]
    classes = {int(k): v for k, v in CLASSES.items()}
    tree = {int(k): v for k, v in TREE4.items()}
    raw = _id_images(41, seed=2)
    present = set(np.unique(raw).tolist())
    assert {3, 1, 6, 7, 11, -1, 41, 46} <= present      # a key that is a value, unmapped, mapped but not in the tree, beyond the table
    for image in raw:
        assert np.array_equal(_lookup(image, table), P.reference_loops(image, classes, tree, 4))
    # class_mapping None: the identity (the "ab" modes); the tree alone decides
    ident = composed_label_table(None, TREE4, 4, device="cpu")
    assert tuple(ident.shape) == (41, 5) and ident[:, 4].tolist() == list(range(41))
    assert np.array_equal(_lookup(raw[1], ident), P.reference_loops(raw[1], None, tree, 4))
    # no tree, no levels: the one-column flat remap ('nyu40')
    flat = composed_label_table(CLASSES, None, 0, device="cpu")
    assert tuple(flat.shape) == (14, 1) and flat[:, 0].tolist() == [0, 3, 5, 9, 4, 5, 6, 40, 8, 9, 10, 11, 1, 0]
    small = _id_images(14, seed=3)[0]
    assert np.array_equal(_lookup(small, flat), P.reference_loops(small, classes, None, 0))
    # with five levels and string keys; of two equal keys the later one wins
    tree5 = {str(k): tuple(v) + (k % 3,) for k, v in tree.items()}
    five = composed_label_table({"1": 3, 1: 4}, tree5, 5, device="cpu")
    assert five[1].tolist() == [2, 0, -1, -1, 1, 4]
    assert np.array_equal(_lookup(raw[2], five), P.reference_loops(raw[2], {1: 4}, {int(k): v for k, v in tree5.items()}, 5))


def test_composed_label_table_errors():
    from hsr_utils import composed_label_table
    with pytest.raises(RuntimeError, match="has 4 levels"):
        composed_label_table(CLASSES, TREE4, 3, device="cpu")
    with pytest.raises(ValueError, match="0..16 levels"):
        composed_label_table(CLASSES, TREE4, 17, device="cpu")
    with pytest.raises(ValueError, match="num_levels"):
        composed_label_table(CLASSES, None, 2, device="cpu")
    with pytest.raises(ValueError, match="num_levels"):
        composed_label_table(CLASSES, TREE4, 0, device="cpu")
    with pytest.raises(RuntimeError, match="empty"):
        composed_label_table(None, None, 0, device="cpu")
    with pytest.raises(RuntimeError, match="not negative"):
        composed_label_table({-1: 2}, None, 0, device="cpu")
    with pytest.raises(RuntimeError, match="not negative"):
        composed_label_table(None, {"-4": (1,)}, 1, device="cpu")
    with pytest.raises(RuntimeError, match="int32"):
        composed_label_table({1: 1 << 31}, None, 0, device="cpu")
    with pytest.raises(RuntimeError, match="too large"):
        composed_label_table({(1 << 24) + 1: 0}, None, 0, device="cpu")


# ---- the tsv readers ------------------------------------------------------------------------------------------------------------------------
# the header line of scannetv2-labels.combined.tsv, and the tree files' further columns as scannet.py:747-778 / :904-947 index them
TSV_HEADER = ["id", "raw_category", "category", "count", "nyu40id", "eigen13id", "nyuClass", "nyu40class", "eigen13class", "ModelNet40",
              "ModelNet10", "ShapeNetCore55", "synsetoffset", "wnsynsetid", "wnsynsetkey", "mpcat40", "mpcat40index"]
TREE_HEADER = TSV_HEADER + [c for l in range(1, 6) for c in ("level%d_id" % l, "level%d" % l)]


def _write_tsv(path, header, rows):
    with open(path, "w") as f:
        for row in [header] + rows:
            f.write("\t".join(str(c) for c in row) + "\n")


def _row(raw_id, nyu_id, levels=(), name="thing"):
    base = [raw_id, name, name, 100, nyu_id, 1, name, "nyu-" + name, "e", "-", "-", "", "", "", "", "objects", 39]
    for l, label in enumerate(levels):
        base += [label, "" if label == "" else "L%d-%s" % (l, label)]
    return base


def test_scannet_class_mapping(tmp_path):
    from hsr_utils import scannet_class_mapping
    path = tmp_path / "scannetv2-labels.combined.tsv"
    _write_tsv(path, TSV_HEADER, [_row(1, 1), _row(2, 5), _row(22, 23), _row(1163, 40), _row(2, 7)])
    assert scannet_class_mapping(str(path)) == {1: 1, 2: 7, 22: 23, 1163: 40}      # the header skipped; the later line of id 2 wins
    assert scannet_class_mapping(str(path), column=5) == {1: 1, 2: 1, 22: 1, 1163: 1}
    _write_tsv(path, TSV_HEADER, [_row(1, 1), [3, "short", "line"]])
    with pytest.raises(RuntimeError, match="line 3 has 3 cells"):
        scannet_class_mapping(str(path))
    _write_tsv(path, TSV_HEADER, [_row(1, "wall")])
    with pytest.raises(ValueError):
        scannet_class_mapping(str(path))


def test_scannet_tree_annotation(tmp_path):
    from hsr_utils import composed_label_table, scannet_tree_annotation
    path = tmp_path / "tree.tsv"
    rows = [_row(5, 3, (1, 0, 2, 0, 4)), _row(2, 1, (0, 1, "", "", "")), _row(9, 3, (1, 0, 2, 1, 0)), _row(7, 8, (2, 5))[:19],      # a short line: it ends before cell 19
            _row(4, 2, (3, "", 6, 2, 1))]                                                                                      # an empty cell inside
    _write_tsv(path, TREE_HEADER, rows)
    tree, num_semantic = scannet_tree_annotation(str(path), 4, key_column=4)      # keyed by the NYU40 id, four levels
    assert list(tree.items()) == [(1, (0, 1, -1, -1)), (2, (3, -1, 6, 2)), (3, (1, 0, 2, 1)), (8, (2, -1, -1, -1))]      # ascending; the later 3 wins
    assert num_semantic == [4, 2, 7, 3, 4]
    tree5, num5 = scannet_tree_annotation(str(path), 5, key_column=0)             # keyed by the raw id, five levels
    assert list(tree5.items()) == [(2, (0, 1, -1, -1, -1)), (4, (3, -1, 6, 2, 1)), (5, (1, 0, 2, 0, 4)), (7, (2, -1, -1, -1, -1)),
                                   (9, (1, 0, 2, 1, 0))]
    assert num5 == [4, 2, 7, 3, 5, 5]
    table = composed_label_table({5: 3, 6: 1}, tree, 4, device="cpu")
    assert tuple(table.shape) == (9, 5) and table[5].tolist() == [1, 0, 2, 1, 3] and table[6].tolist() == [0, 1, -1, -1, 1]
    with pytest.raises(ValueError, match="at least one level"):
        scannet_tree_annotation(str(path), 0, key_column=4)
    _write_tsv(path, TREE_HEADER, [["1", "a"]])
    with pytest.raises(RuntimeError, match="key column 4"):
        scannet_tree_annotation(str(path), 4, key_column=4)
    _write_tsv(path, TREE_HEADER, [])
    with pytest.raises(RuntimeError, match="names no class"):
        scannet_tree_annotation(str(path), 4, key_column=4)
    assert "restated, not pinned by a file of the dataset" in " ".join(scannet_tree_annotation.__doc__.lower().split())


# ---- the ScanNet-layout reader ------------------------------------------------------------------------------------------------------------
HC, WC, HD, WD = 20, 26, 10, 13
NUMBERS = (9, 10, 11, 12, 100)      # 9.jpg before 10.jpg and 100.jpg last: the order of the integers, not of the characters
LOST = 2                            # the frame whose pose file holds -inf


def _pose(k):
    a, b = 0.25 + 0.15 * k, 0.1 * k
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    m = np.eye(4)
    m[:3, :3] = rz @ ry
    m[:3, 3] = [1.5 - 0.1 * k, 0.2 * k, 0.7 + 0.03 * k * k]
    return m


def _write_pose(path, m):
    with open(path, "w") as f:
        for row in m:
            f.write(" ".join("-inf" if v == -np.inf else repr(float(v)) for v in row) + "\n")


@pytest.fixture(scope="module")
def scannet_dir(tmp_path_factory):
    from PIL import Image
    base = tmp_path_factory.mktemp("scannet")
    seq = base / "scene0000_00"
    for sub in ("color", "depth", "pose", "label-filt"):
        (seq / sub).mkdir(parents=True)
    g = np.random.default_rng(11)
    written = []
    for k, number in enumerate(NUMBERS):
        smooth = np.add.outer(np.arange(HC) * 7, np.arange(WC) * 4)[..., None] + np.array([12 * k, 50, 110])
        col = smooth.astype(np.uint8)
        dep = g.integers(0, 65536, size=(HD, WD)).astype(np.uint16)
        dep[0, 0], dep[0, 1] = 0, 65535
        lab = g.integers(0, 1400, size=(HC, WC)).astype(np.uint16)      # raw ScanNet ids go beyond 8 bits
        lab[0, 0], lab[0, 1] = 0, 65535
        Image.fromarray(col).save(seq / "color" / ("%d.jpg" % number), quality=95)
        Image.fromarray(dep).save(seq / "depth" / ("%d.png" % number))
        Image.fromarray(lab).save(seq / "label-filt" / ("%d.png" % number))
        _write_pose(seq / "pose" / ("%d.txt" % number), np.full((4, 4), -np.inf) if k == LOST else _pose(k))
        written.append((number, dep, lab))
    return str(base), written


def test_scannet_sequence_reads_what_was_written(scannet_dir):
    from PIL import Image
    from hsr_utils import ScanNetSequence
    base, written = scannet_dir
    seq = ScanNetSequence(base, "scene0000_00")
    assert len(seq) == 5 and seq.retained_inds == [0, 1, 2, 3, 4]
    for paths, ext in ((seq.color_paths, "jpg"), (seq.depth_paths, "png"), (seq.pose_paths, "txt"), (seq.label_paths, "png")):
        assert [os.path.basename(p) for p in paths] == ["%d.%s" % (n, ext) for n in NUMBERS]
    first_inv = np.linalg.inv(_pose(0))
    for i, (number, dep, lab) in enumerate(written):
        color, depth, labels, gt_w2c = seq[i]
        assert color.dtype == np.uint8 and color.shape == (HC, WC, 3) and color.flags["C_CONTIGUOUS"]
        with Image.open(os.path.join(base, "scene0000_00", "color", "%d.jpg" % number)) as im:
            assert np.array_equal(color, np.asarray(im))                                 # JPEG: what PIL decodes from the file
        assert depth.dtype == np.uint16 and depth.shape == (HD, WD) and np.array_equal(depth, dep)      # PNG: bit for bit what was written
        assert labels.dtype == np.int32 and labels.shape == (HC, WC) and np.array_equal(labels, lab.astype(np.int32))
        assert labels.flags["C_CONTIGUOUS"] and depth.flags["C_CONTIGUOUS"]
        assert gt_w2c.dtype == np.float32 and gt_w2c.shape == (4, 4)
        if i == LOST:
            assert np.isnan(gt_w2c).all()                                                # a lost pose: NaN, never a keyframe
        else:
            want = np.linalg.inv(first_inv @ _pose(i))                                   # relative to the first frame, then inverted
            assert np.array_equal(gt_w2c, want.astype(np.float32))
            assert np.abs(gt_w2c - (np.linalg.inv(_pose(i)) @ _pose(0))).max() <= 1e-6
    assert np.abs(seq[0][3] - np.eye(4)).max() <= 1e-7 and np.abs(seq[1][3] - np.eye(4)).max() > 0.05
    assert np.array_equal(seq[-1][1], written[4][1])
    with pytest.raises(IndexError):
        seq[5]
    assert len(list(seq)) == 5
    bare = ScanNetSequence(base, "scene0000_00", labels=False)
    assert bare.label_paths is None and bare[3][2] is None and np.array_equal(bare[3][1], written[3][1])


def test_scannet_sequence_start_end_stride(scannet_dir):
    from hsr_utils import ScanNetSequence
    base, written = scannet_dir
    seq = ScanNetSequence(base, "scene0000_00", start=1, end=-1, stride=2)
    assert len(seq) == 2 and seq.retained_inds == [1, 3]
    assert np.array_equal(seq[0][1], written[1][1]) and np.array_equal(seq[1][2], written[3][2].astype(np.int32))
    assert np.abs(seq[0][3] - np.eye(4)).max() <= 1e-7      # relative to the first RETAINED frame
    assert np.array_equal(seq[1][3], np.linalg.inv(np.linalg.inv(_pose(1)) @ _pose(3)).astype(np.float32))
    seq = ScanNetSequence(base, "scene0000_00", start=0, end=3)
    assert seq.retained_inds == [0, 1, 2] and os.path.basename(seq.color_paths[-1]) == "11.jpg" and np.isnan(seq[2][3]).all()
    assert ScanNetSequence(base, "scene0000_00", start=3, end=4, stride=5).retained_inds == [3]
    for kw in (dict(start=-1), dict(start=2, end=2), dict(start=3, end=1), dict(stride=0)):
        with pytest.raises(ValueError, match="hsr_utils.sequence"):
            ScanNetSequence(base, "scene0000_00", **kw)
    with pytest.raises(RuntimeError, match="no frame"):
        ScanNetSequence(base, "scene0000_00", start=7)
    with pytest.raises(RuntimeError, match=r"color/\*.jpg"):
        ScanNetSequence(base, "nowhere")
    # a sequence that would start at the lost pose has nothing to be relative to
    with pytest.raises(RuntimeError, match=r"pose.11\.txt, the first retained pose, is not finite"):
        ScanNetSequence(base, "scene0000_00", start=LOST)


def test_scannet_sequence_error_paths(tmp_path):
    from PIL import Image
    from hsr_utils import ScanNetSequence
    seq = tmp_path / "s"
    for sub in ("color", "depth", "pose", "label-filt"):
        (seq / sub).mkdir(parents=True)
    col, dep, lab = np.zeros((4, 6, 3), np.uint8), np.zeros((2, 3), np.uint16), np.zeros((4, 6), np.uint16)
    for n in (0, 1):
        Image.fromarray(col).save(seq / "color" / ("%d.jpg" % n))
    Image.fromarray(dep).save(seq / "depth" / "0.png")
    with pytest.raises(RuntimeError, match=r"2 color/\*.jpg and 1 depth/\*.png"):
        ScanNetSequence(str(tmp_path), "s")
    Image.fromarray(dep).save(seq / "depth" / "1.png")
    _write_pose(seq / "pose" / "0.txt", np.eye(4))
    with pytest.raises(RuntimeError, match="1 poses for 2 frames"):
        ScanNetSequence(str(tmp_path), "s")
    with open(seq / "pose" / "1.txt", "w") as f:
        f.write("1 0 0 0\n0 1 0 0\n0 0 1\n")
    Image.fromarray(lab).save(seq / "label-filt" / "0.png")
    with pytest.raises(RuntimeError, match="label-filt holds 1 images for 2 frames"):
        ScanNetSequence(str(tmp_path), "s")
    with pytest.raises(RuntimeError, match=r"1\.txt has 11 numbers, not 16"):
        ScanNetSequence(str(tmp_path), "s", labels=False)
    _write_pose(seq / "pose" / "1.txt", np.eye(4))
    Image.fromarray(np.zeros((4, 6, 3), np.uint8)).save(seq / "label-filt" / "1.png")      # three channels: not a label image
    ok = ScanNetSequence(str(tmp_path), "s")
    assert ok[0][2].shape == (4, 6) and ok[0][1].shape == (2, 3)
    with pytest.raises(RuntimeError, match="not a one-channel integer image"):
        ok[1]
    Image.fromarray(np.zeros((2, 3, 3), np.uint8)).save(seq / "depth" / "1.png")
    with pytest.raises(RuntimeError, match="not a one-channel image"):
        ok[1]
    Image.fromarray(np.zeros((4, 6), np.uint8)).save(seq / "color" / "1.jpg")               # grey: not a colour image
    with pytest.raises(RuntimeError, match="not an 8-bit three-channel image"):
        ok[1]


# ---- argument errors that need no device -------------------------------------------------------------------------------------------------
def test_ingest_frame_planes_argument_errors():
    from hsr_utils import ingest_frame_planes
    from hsr_utils.frames import ingest_frame_planes as from_frames
    assert ingest_frame_planes is from_frames
    col, _same = I.make_frame(4, 6)
    _c, dep = I.make_frame(3, 5)
    lab = np.zeros((7, 2), dtype=np.uint8)
    table = torch.zeros((3, 2), dtype=torch.int32)
    for bad_color in (col.astype(np.float32), col[..., :2], col[0], torch.zeros(3, 4, 6, dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match="color_u8 must be"):
            ingest_frame_planes(bad_color, dep, [(2, 3)], 1000.0)
    for bad_depth in (dep.astype(np.float64), dep.astype(np.int64), dep.astype(np.uint8)):
        with pytest.raises(RuntimeError, match="depth_raw must be uint16"):
            ingest_frame_planes(col, bad_depth, [(2, 3)], 1000.0)
    for bad_depth in (dep[0], dep[None]):
        with pytest.raises(RuntimeError, match="depth_raw must be a 2-D"):
            ingest_frame_planes(col, bad_depth, [(2, 3)], 1000.0)
    for bad_labels in (lab.astype(np.float32), lab[0], lab[None], torch.zeros(4, 6, dtype=torch.bool)):
        with pytest.raises(RuntimeError, match="labels must be an integer"):
            ingest_frame_planes(col, dep, [(2, 3)], 1000.0, labels=bad_labels)
    with pytest.raises(RuntimeError, match="label_table without labels"):
        ingest_frame_planes(col, dep, [(2, 3)], 1000.0, label_table=table)
    with pytest.raises(RuntimeError, match="leaf_column without a label_table"):
        ingest_frame_planes(col, dep, [(2, 3)], 1000.0, labels=lab, leaf_column=True)
    for bad_table in (table.long(), table[0], table.numpy(), torch.zeros((0, 2), dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="label_table must be an int32 2-D"):
            ingest_frame_planes(col, dep, [(2, 3)], 1000.0, labels=lab, label_table=bad_table)
    for bad_table, leaf in ((torch.zeros((3, 0), dtype=torch.int32), False), (torch.zeros((3, 17), dtype=torch.int32), False),
                            (torch.zeros((3, 18), dtype=torch.int32), True), (torch.zeros((3, 0), dtype=torch.int32), True)):
        with pytest.raises(RuntimeError, match="level columns"):
            ingest_frame_planes(col, dep, [(2, 3)], 1000.0, labels=lab, label_table=bad_table, leaf_column=leaf)
    for bad_sizes in ([], [(2, 3)] * 4, [(0, 3)], [(2, 16385)], [(2, 3), (2, 3), (-1, 3)]):
        with pytest.raises(ValueError, match="ingest_frame_planes"):
            ingest_frame_planes(col, dep, bad_sizes, 1000.0)
    with pytest.raises(ValueError, match="ingest_frame_planes sides"):
        ingest_frame_planes(col, np.zeros((0, 5), np.uint16), [(2, 3)], 1000.0)
    for bad_scale in (0, 0.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="png_depth_scale"):
            ingest_frame_planes(col, dep, [(2, 3)], bad_scale)
    if not torch.cuda.is_available():      # well-formed calls, among them a one-column table with leaf_column, get as far as the device
        for kw in (dict(), dict(labels=lab), dict(labels=lab, label_table=table), dict(labels=lab, label_table=table[:, :1], leaf_column=True)):
            with pytest.raises(RuntimeError, match="no CPU path"):
                ingest_frame_planes(col, dep, [(2, 3)], 1000.0, **kw)


# ---- SlamSession.ingest: which of the two functions a frame goes to ---------------------------------------------------------------------
def test_session_ingest_routing(monkeypatch):
    import test_frame_ingest_cpu as T
    from hsr_utils import frames, slam
    assert list(inspect.signature(slam.SlamSession.ingest).parameters)[-1] == "leaf_column"
    assert inspect.signature(slam.SlamSession.ingest).parameters["leaf_column"].default is False
    col, dep = I.make_frame(4, 6)
    lab = np.zeros((4, 6), np.uint8)
    small_dep, small_lab = I.make_frame(3, 5)[1], np.zeros((3, 5), np.uint8)
    table = torch.zeros((3, 2), dtype=torch.int32)
    seen = []

    def result(sizes, labels):
        out = [(torch.zeros(3, h, w), torch.zeros(1, h, w)) for h, w in sizes]
        return out, (None if labels is None else torch.zeros((1,) + tuple(sizes[0]), dtype=torch.int64))

    def fake(color_u8, depth_raw, sizes, scale, labels=None, tree_table=None):
        seen.append(("ingest_frame", color_u8, depth_raw, list(sizes), scale, labels, tree_table))
        return result(sizes, labels)

    def fake_planes(color_u8, depth_raw, sizes, scale, labels=None, label_table=None, leaf_column=False):
        seen.append(("ingest_frame_planes", color_u8, depth_raw, list(sizes), scale, labels, label_table, leaf_column))
        return result(sizes, labels)
    monkeypatch.setattr(frames, "ingest_frame", fake)
    monkeypatch.setattr(frames, "ingest_frame_planes", fake_planes)
    s = slam.SlamSession(T._config(data=dict(num_frames=8, png_depth_scale=1000.0)), torch.eye(3), torch.eye(4), cam=T._Cam())
    # equal shapes: ingest_frame with today's arguments, numpy arrays and tensors alike
    frame = s.ingest(1, col, dep, labels=lab, tree_table=table)
    assert len(seen) == 1 and seen[-1][0] == "ingest_frame" and seen[-1][1] is col and seen[-1][2] is dep
    assert seen[-1][3:5] == ([(4, 6)], 1000.0) and seen[-1][5] is lab and seen[-1][6] is table
    assert set(frame) == {"id", "im", "depth", "semantic_label_gt"}
    s.ingest(1, torch.from_numpy(col), torch.from_numpy(dep.view(np.int16)))
    assert seen[-1][0] == "ingest_frame" and seen[-1][5] is None and seen[-1][6] is None
    s.ingest(1, col[..., :2], dep)      # colour that cannot be read as [H,W,3] is ingest_frame's to refuse, as before
    assert seen[-1][0] == "ingest_frame"
    # a depth of another size
    gt = np.eye(4, dtype=np.float32)
    frame = s.ingest(2, col, small_dep, gt_w2c=gt, labels=lab, tree_table=table)
    assert seen[-1][0] == "ingest_frame_planes" and seen[-1][1] is col and seen[-1][2] is small_dep and seen[-1][3:5] == ([(4, 6)], 1000.0)
    assert seen[-1][5] is lab and seen[-1][6] is table and seen[-1][7] is False
    assert set(frame) == {"id", "im", "depth", "gt_w2c", "semantic_label_gt"} and frame["id"] == 2 and frame["gt_w2c"] is gt
    s.ingest(2, col, torch.from_numpy(small_dep.view(np.int16)))
    assert seen[-1][0] == "ingest_frame_planes" and seen[-1][5] is None
    # labels of another size
    s.ingest(3, col, dep, labels=small_lab, png_depth_scale=5000.0)
    assert seen[-1][0] == "ingest_frame_planes" and seen[-1][4] == 5000.0 and seen[-1][5] is small_lab and seen[-1][7] is False
    # leaf_column with equal shapes
    s.ingest(4, col, dep, labels=lab, tree_table=table, leaf_column=True)
    assert seen[-1][0] == "ingest_frame_planes" and seen[-1][6] is table and seen[-1][7] is True
    assert len(seen) == 7
