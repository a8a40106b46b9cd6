"""CPU suite for the ingest of raw sensor frames: the prototype of include/ext/hsr_frame_ingest.h (its name, type classes and level
structure; tests/test_abi.py checks that it is exported and bound with the header's types), its argument checks, the numpy restatement of the header
(tests/ingest_ref.py) against the two independent float64 restatements of tests/resample_ref.py, tree_label_table, the Replica-layout
reader of hsr_utils.sequence on a directory the test writes, and the argument errors of ingest_frame and SlamSession.ingest that need
no device.  Nothing here launches: there is no GPU."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import ingest_ref as I
import resample_ref as R
import test_abi

EXT_HEADER = "ext/hsr_frame_ingest.h"
IDS = ["%dx%d-%dx%d" % (s + d) for s, d in R.SIZE_PAIRS]


def test_frame_ingest_abi_exported_and_bound():
    from diff_gaussian_rasterization import _abi
    protos = test_abi._prototypes([EXT_HEADER])
    assert [s[0] for s in _abi.HEADERS[EXT_HEADER]] == list(protos) == ["hsr_frame_ingest"]
    assert protos["hsr_frame_ingest"][2][5] == "double" and protos["hsr_frame_ingest"][2][11] == ("pointer", "hsr_ingest_level")
    # the structure carries the field names of its typedef, in order, and the C layout
    structs = test_abi._structures([EXT_HEADER])
    assert list(structs) == ["hsr_ingest_level"]
    assert structs["hsr_ingest_level"] == [f[0] for f in _abi.hsr_ingest_level._fields_] == ["H", "W", "color", "depth"]
    assert C.sizeof(_abi.hsr_ingest_level) == 24
    from hsr_utils import evaluate, frames, slam
    defines = dict(re.findall(r"^#define\s+(HSR_\w+)\s+(\d+)\s*$", test_abi._source(EXT_HEADER), flags=re.M))
    assert frames.INGEST_MAX_LEVELS == int(defines["HSR_INGEST_MAX_LEVELS"]) == 3
    assert (frames.DEPTH_U16, frames.DEPTH_I32, frames.DEPTH_F32) == tuple(
        int(defines["HSR_INGEST_DEPTH_" + k]) for k in ("U16", "I32", "F32")) == (0, 1, 2)
    assert frames.INGEST_MAX_SIDE == slam.RESAMPLE_MAX_SIDE and frames.INGEST_MAX_TREE_LEVELS == evaluate.MAX_LEVELS


def test_frame_ingest_refuses_before_any_device_work():
    """bad sizes, counts, scales and NULL pointers are an error code and a message, not a launch (no pointer here is a device pointer)"""
    from diff_gaussian_rasterization import _abi
    lib = _abi.lib
    fake = 4096      # never dereferenced: every call below is refused before the launch

    def call(Hs=8, Ws=8, color=fake, depth=fake, depth_type=0, scale=1000.0, labels=None, L=0, table=None, n_ids=0, n_out=1,
             sizes=((4, 4),), outs=(fake, fake), out_labels=None, levels="array"):
        arr = (_abi.hsr_ingest_level * 4)(*[_abi.hsr_ingest_level(h, w, outs[0], outs[1]) for h, w in (tuple(sizes) + ((4, 4),) * 4)[:4]])
        return lib.hsr_frame_ingest(Hs, Ws, color, depth, depth_type, scale, labels, L, table, n_ids, n_out, arr if levels == "array" else None,
                                    out_labels, None)
    for kw in (dict(Hs=0), dict(Ws=16385), dict(Hs=-2), dict(sizes=((0, 4),)), dict(sizes=((4, 16385),)),
               dict(n_out=2, sizes=((4, 4), (16385, 4))), dict(n_out=3, sizes=((4, 4), (4, 4), (4, 0)))):
        assert call(**kw) == -1 and b"frame_ingest: sides" in lib.hsr_last_error(), kw
    for kw in (dict(n_out=0), dict(n_out=4), dict(n_out=-1), dict(levels=None)):
        assert call(**kw) == -1 and b"frame_ingest: n_out" in lib.hsr_last_error(), kw
    for kw in (dict(depth_type=3), dict(depth_type=-1)):
        assert call(**kw) == -1 and b"frame_ingest: depth_type" in lib.hsr_last_error(), kw
    for kw in (dict(scale=0.0), dict(scale=-0.0), dict(scale=float("inf")), dict(scale=float("nan"))):
        assert call(**kw) == -1 and b"frame_ingest: depth_scale" in lib.hsr_last_error(), kw
    for kw in (dict(L=-1), dict(L=17, table=fake, n_ids=4), dict(L=2, labels=fake, out_labels=fake), dict(L=2, table=fake, n_ids=0, labels=fake, out_labels=fake)):
        assert call(**kw) == -1 and b"frame_ingest: num_levels" in lib.hsr_last_error(), kw
    for kw in (dict(color=None), dict(depth=None), dict(outs=(None, fake)), dict(outs=(fake, None)), dict(labels=fake), dict(out_labels=fake),
               dict(Hs=16384, Ws=16384, color=None, n_out=3, sizes=((16384, 16384), (1, 16384), (16384, 1)))):
        assert call(**kw) == -1 and b"frame_ingest: NULL" in lib.hsr_last_error(), kw


@pytest.mark.parametrize("src,dst", R.SIZE_PAIRS, ids=IDS)
def test_in_order_colour_agrees_with_both_independent_restatements(src, dst):
    """v of the header's order of operations against F.interpolate and map_coordinates on float64(u8), in grey levels.  1e-10: the
    three differ only in the order of float64 operations on values <= 255 (ulp 2.8e-14, a handful of roundings each; 2.3e-12 was
    measured), so the bound is a float64 rounding allowance forty times the measured figure, not a fit."""
    col, _dep = I.make_frame(*src, seed=7 * src[0] + dst[1])
    v = I.color_v(col, dst)
    vt, vs = I.independent_v(col, dst)
    assert v.shape == vt.shape == vs.shape == (3,) + dst and v.dtype == vt.dtype == vs.dtype == np.float64
    dist = max(float(np.abs(v - vt).max()), float(np.abs(v - vs).max()))
    print("ingest_ref %dx%d -> %dx%d: in-order v vs torch / scipy on float64(u8): %.3g grey levels" % (src + dst + (dist,)))
    assert dist <= 1e-10
    out = I.color(col, dst)
    assert out.dtype == np.float32 and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    if src == dst:      # fx = fy = 0: float32(g) / float32(255) exactly
        assert np.array_equal(v, col.transpose(2, 0, 1).astype(np.float64))
        assert np.array_equal(out, col.transpose(2, 0, 1).astype(np.float32) / np.float32(255))
    if src == (16, 16):      # exact 2x: the mean of each 2x2 block
        assert np.array_equal(v, col.transpose(2, 0, 1).astype(np.float64).reshape(3, 8, 2, 8, 2).mean(axis=(2, 4)))


def test_division_through_double_is_the_fp32_division():
    """the header's allowed equivalent: float(double(float(v)) / 255.0) == float(v) / 255.0f, on all grey levels and random values"""
    g = np.random.default_rng(0)
    v = np.concatenate([np.arange(256, dtype=np.float32), (g.random(200000) * 255).astype(np.float32)])
    assert np.array_equal(v / np.float32(255), (v.astype(np.float64) / 255.0).astype(np.float32))


def test_depth_and_label_restatements():
    _col, dep = I.make_frame(5, 7, seed=1)
    assert np.array_equal(I.depth(dep, (5, 7), 1.0), dep.astype(np.float32))
    assert np.array_equal(I.depth(dep, (2, 3), 1000.0), (dep[[0, 2]][:, [0, 2, 4]].astype(np.float64) / 1000.0).astype(np.float32))
    f = np.array([[0.0, np.nan], [np.inf, 2.0]], dtype=np.float32)
    out = I.depth(f, (2, 2), 2.0)
    assert out[0, 0] == 0 and np.isnan(out[0, 1]) and np.isinf(out[1, 0]) and out[1, 1] == 1.0
    ids = np.array([[0, 1, 2], [5, -1, 1]], dtype=np.int32)
    table = np.array([[7, 8], [-1, 9], [2, 2]], dtype=np.int32)
    got = I.labels(ids, (2, 3), table)
    assert got.dtype == np.int64 and got.tolist() == [[[7, -1, 2], [5, -1, -1]], [[8, 9, 2], [5, -1, 9]], [[0, 1, 2], [5, -1, 1]]]
    assert I.labels(ids, (1, 2), None).tolist() == [[[0, 1]]]


def test_tree_label_table():
    from hsr_utils import tree_label_table
    from hsr_utils.frames import tree_label_table as from_frames
    assert tree_label_table is from_frames
    tree = {"0": (0, 0, 1), 2: (1, -1, 4), "5": (2, 3, 0), "2": (1, 2, 3)}      # "2" after 2: the later key wins
    t = tree_label_table(tree, 3, device="cpu")
    assert t.dtype == torch.int32 and tuple(t.shape) == (6, 3)
    assert t.tolist() == [[0, 0, 1], [1, 1, 1], [1, 2, 3], [3, 3, 3], [4, 4, 4], [2, 3, 0]]      # rows 1, 3, 4: their own id
    assert tree_label_table({2: (1, 2, 3), "2": (1, -1, 4)}, 3, device="cpu")[2].tolist() == [1, -1, 4]
    with pytest.raises(RuntimeError, match="has 2 levels"):
        tree_label_table({1: (0, 1)}, 3, device="cpu")
    with pytest.raises(ValueError, match="1..16 levels"):
        tree_label_table({1: ()}, 0, device="cpu")
    with pytest.raises(RuntimeError, match="empty"):
        tree_label_table({}, 2, device="cpu")
    # the restatement, given the table, keeps an unknown class's id on every level
    ids = np.array([[1, 9, 2, -3]], dtype=np.int64)
    assert I.labels(ids, (1, 4), t.numpy()).tolist() == [[[1, 9, 1, -3]], [[1, 9, 2, -3]], [[1, 9, 3, -3]], [[1, 9, 2, -3]]]


# ---- the Replica-layout reader ---------------------------------------------------------------------------------------------------------
SEQ_H, SEQ_W = 6, 8
SEQ_NUMBERS = (0, 5, 9, 10)      # frame9 before frame10: the order of the integers, not of the characters


def _pose(k):
    """a rigid camera-to-world matrix; that of frame 0 is not the identity"""
    a, b = 0.3 + 0.2 * k, -0.1 * k
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    m = np.eye(4)
    m[:3, :3] = rz @ rx
    m[:3, 3] = [0.5 + 0.1 * k, -0.2 * k, 1.0 + 0.05 * k * k]
    return m


@pytest.fixture(scope="module")
def replica_dir(tmp_path_factory):
    from PIL import Image
    base = tmp_path_factory.mktemp("replica")
    seq, sem = base / "data" / "room9", base / "sem" / "room9"
    (seq / "results").mkdir(parents=True)
    (sem / "semantic_class").mkdir(parents=True)
    g = np.random.default_rng(3)
    written = []
    for k, number in enumerate(SEQ_NUMBERS):
        smooth = np.add.outer(np.arange(SEQ_H) * 9, np.arange(SEQ_W) * 5)[..., None] + np.array([10 * k, 60, 120])
        col = smooth.astype(np.uint8)
        dep = g.integers(0, 65536, size=(SEQ_H, SEQ_W)).astype(np.uint16)
        dep[0, 0], dep[0, 1] = 0, 65535
        lab = g.integers(0, 102, size=(SEQ_H, SEQ_W)).astype(np.uint8)
        Image.fromarray(col).save(seq / "results" / ("frame%d.jpg" % number), quality=95)
        Image.fromarray(dep).save(seq / "results" / ("depth%d.png" % number))
        Image.fromarray(lab).save(sem / "semantic_class" / ("semantic_class_%d.png" % number))
        written.append((number, dep, lab))
    with open(seq / "traj.txt", "w") as f:
        for k in range(len(SEQ_NUMBERS)):
            f.write(" ".join(repr(float(v)) for v in _pose(k).reshape(-1)) + "\n")
    tree = {"0_undefined": [{"0": "void"}], "3_chair": [{"1": "furniture"}, {"2": "seat"}, {"0": "chair"}],
            "7_table": [{"1": "furniture"}, {"0": "surface"}], "12_wall": [{"2": "structure"}, {"1": "wall"}, {"4": "plain wall"}]}
    with open(sem / "info_semantic_tree.json", "w") as f:
        json.dump(tree, f)
    return str(base / "data"), str(base / "sem"), written


def test_replica_sequence_reads_what_was_written(replica_dir):
    from PIL import Image
    from hsr_utils import ReplicaSequence
    data, sem, written = replica_dir
    seq = ReplicaSequence(data, "room9", semantic_dir=sem)
    assert len(seq) == 4 and seq.retained_inds == [0, 1, 2, 3]
    assert [os.path.basename(p) for p in seq.color_paths] == ["frame%d.jpg" % n for n in SEQ_NUMBERS]      # frame9 before frame10
    assert [os.path.basename(p) for p in seq.depth_paths] == ["depth%d.png" % n for n in SEQ_NUMBERS]
    assert [os.path.basename(p) for p in seq.semantic_paths] == ["semantic_class_%d.png" % n for n in SEQ_NUMBERS]
    first_inv = np.linalg.inv(_pose(0))
    for i, (number, dep, lab) in enumerate(written):
        color, depth, labels, gt_w2c = seq[i]
        assert color.dtype == np.uint8 and color.shape == (SEQ_H, SEQ_W, 3) and color.flags["C_CONTIGUOUS"]
        with Image.open(os.path.join(data, "room9", "results", "frame%d.jpg" % number)) as im:
            assert np.array_equal(color, np.asarray(im))                                 # JPEG: what PIL decodes from the file
        assert depth.dtype == np.uint16 and np.array_equal(depth, dep)                   # PNG: bit for bit what was written
        assert labels.dtype.kind in "iu" and np.array_equal(labels, lab)
        want = np.linalg.inv(first_inv @ _pose(i))                                       # relative to the first frame, then inverted
        assert gt_w2c.dtype == np.float32 and gt_w2c.shape == (4, 4) and np.array_equal(gt_w2c, want.astype(np.float32))
        assert np.abs(gt_w2c - (np.linalg.inv(_pose(i)) @ _pose(0))).max() <= 1e-6      # = w2c_i @ c2w_0
    assert np.array_equal(seq[0][3], np.eye(4, dtype=np.float32)) or np.abs(seq[0][3] - np.eye(4)).max() <= 1e-7
    assert np.abs(seq[1][3] - np.eye(4)).max() > 0.05
    assert np.array_equal(seq[-1][1], written[3][1])
    with pytest.raises(IndexError):
        seq[4]
    assert len(list(seq)) == 4
    bare = ReplicaSequence(data, "room9")
    assert bare[2][2] is None and np.array_equal(bare[2][1], written[2][1])


def test_replica_sequence_start_end_stride(replica_dir):
    from hsr_utils import ReplicaSequence
    data, sem, written = replica_dir
    seq = ReplicaSequence(data, "room9", start=1, end=-1, stride=2, semantic_dir=sem)
    assert len(seq) == 2 and seq.retained_inds == [1, 3]
    assert np.array_equal(seq[0][1], written[1][1]) and np.array_equal(seq[1][1], written[3][1]) and np.array_equal(seq[1][2], written[3][2])
    # the poses are relative to the first RETAINED frame
    assert np.abs(seq[0][3] - np.eye(4)).max() <= 1e-7
    assert np.array_equal(seq[1][3], np.linalg.inv(np.linalg.inv(_pose(1)) @ _pose(3)).astype(np.float32))
    seq = ReplicaSequence(data, "room9", start=0, end=3)
    assert seq.retained_inds == [0, 1, 2] and os.path.basename(seq.color_paths[-1]) == "frame9.jpg"
    seq = ReplicaSequence(data, "room9", start=2, end=3, stride=5)
    assert seq.retained_inds == [2]
    for kw in (dict(start=-1), dict(start=2, end=2), dict(start=2, end=1), dict(stride=0)):
        with pytest.raises(ValueError, match="hsr_utils.sequence"):
            ReplicaSequence(data, "room9", **kw)
    with pytest.raises(RuntimeError, match="no frame"):
        ReplicaSequence(data, "room9", start=7)
    with pytest.raises(RuntimeError, match="frame\\*.jpg"):
        ReplicaSequence(data, "nowhere")


def test_tree_annotation(replica_dir):
    from hsr_utils import tree_annotation, tree_label_table
    _data, sem, _written = replica_dir
    tree, num_semantic = tree_annotation(os.path.join(sem, "room9", "info_semantic_tree.json"), 3)
    assert list(tree.items()) == [("0", (0, -1, -1)), ("3", (1, 2, 0)), ("7", (1, 0, -1)), ("12", (2, 1, 4))]
    assert num_semantic == [3, 3, 5, 4]      # the largest label of each level + 1, then the number of classes
    table = tree_label_table(tree, 3, device="cpu")
    assert tuple(table.shape) == (13, 3) and table[7].tolist() == [1, 0, -1] and table[5].tolist() == [5, 5, 5]
    tree4, num4 = tree_annotation(os.path.join(sem, "room9", "info_semantic_tree.json"), 4)
    assert tree4["3"] == (1, 2, 0, -1) and num4 == [3, 3, 5, 0, 4]
    with pytest.raises(RuntimeError, match="has 3 levels"):
        tree_annotation(os.path.join(sem, "room9", "info_semantic_tree.json"), 2)


# ---- argument errors that need no device -------------------------------------------------------------------------------------------------
def test_ingest_frame_argument_errors():
    from hsr_utils import ingest_frame
    col, dep = I.make_frame(4, 6)
    lab = np.zeros((4, 6), dtype=np.uint8)
    table = torch.zeros((3, 2), dtype=torch.int32)
    for bad_color in (col.astype(np.float32), col[..., :2], col[0], torch.zeros(3, 4, 6, dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match="color_u8 must be"):
            ingest_frame(bad_color, dep, [(2, 3)], 1000.0)
    for bad_depth in (dep.astype(np.float64), dep.astype(np.int64), dep.astype(np.uint8)):
        with pytest.raises(RuntimeError, match="depth_raw must be uint16"):
            ingest_frame(col, bad_depth, [(2, 3)], 1000.0)
    for bad_depth in (dep[:3], dep[None], dep.astype(np.float32)[:, :5]):
        with pytest.raises(RuntimeError, match=r"depth_raw must be \[Hs,Ws\]"):
            ingest_frame(col, bad_depth, [(2, 3)], 1000.0)
    for bad_labels in (lab.astype(np.float32), lab[:3], torch.zeros(4, 6, dtype=torch.bool)):
        with pytest.raises(RuntimeError, match="labels must be an integer"):
            ingest_frame(col, dep, [(2, 3)], 1000.0, labels=bad_labels)
    with pytest.raises(RuntimeError, match="tree_table without labels"):
        ingest_frame(col, dep, [(2, 3)], 1000.0, tree_table=table)
    for bad_table in (table.long(), table[0], torch.zeros((3, 17), dtype=torch.int32), table.numpy()):
        with pytest.raises(RuntimeError, match="tree_table must be an int32"):
            ingest_frame(col, dep, [(2, 3)], 1000.0, labels=lab, tree_table=bad_table)
    for bad_sizes in ([], [(2, 3)] * 4, [(0, 3)], [(2, 16385)], [(2, 3), (2, 3), (-1, 3)]):
        with pytest.raises(ValueError, match="ingest_frame"):
            ingest_frame(col, dep, bad_sizes, 1000.0)
    for bad_scale in (0, 0.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="png_depth_scale"):
            ingest_frame(col, dep, [(2, 3)], bad_scale)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            ingest_frame(col, dep, [(2, 3)], 1000.0, labels=lab, tree_table=table)


def _config(**over):
    lrs = dict(means3D=0.0, rgb_colors=0.0, unnorm_rotations=0.0, logit_opacities=0.0, log_scales=0.0, cam_unnorm_rots=4e-4, cam_trans=2e-3)
    cfg = dict(map_every=1, keyframe_every=3, mapping_window_size=4, data=dict(num_frames=8),
               tracking=dict(num_iters=5, lrs=lrs, loss_weights=dict(im=0.5, depth=1.0), sil_thres=0.99),
               mapping=dict(num_iters=5, lrs=lrs, loss_weights=dict(im=0.5, depth=1.0), sil_thres=0.5))
    cfg.update(over)
    return cfg


class _Cam:
    image_height, image_width = 4, 6


def test_session_ingest_argument_errors(monkeypatch):
    from hsr_utils import frames, slam
    col, dep = I.make_frame(4, 6)
    s = slam.SlamSession(_config(), torch.eye(3), torch.eye(4), cam=_Cam())
    with pytest.raises(KeyError, match="png_depth_scale"):
        s.ingest(0, col, dep)
    with pytest.raises(RuntimeError, match="color_u8 must be"):
        s.ingest(0, col[..., :2], dep, png_depth_scale=1000.0)
    with pytest.raises(ValueError, match="png_depth_scale"):
        s.ingest(0, col, dep, png_depth_scale=0.0)
    # the scale comes from config['data'], the top level winning, and the explicit argument over both; one call with the frame's size
    seen = []

    def fake(color_u8, depth_raw, sizes, scale, labels=None, tree_table=None):
        seen.append((list(sizes), scale, labels is not None))
        out = [(torch.zeros(3, h, w), torch.zeros(1, h, w)) for h, w in sizes]
        return out, (None if labels is None else torch.zeros((1,) + tuple(sizes[0]), dtype=torch.int64))
    monkeypatch.setattr(frames, "ingest_frame", fake)
    s = slam.SlamSession(_config(data=dict(num_frames=8, png_depth_scale=6553.5)), torch.eye(3), torch.eye(4), cam=_Cam())
    frame = s.ingest(2, col, dep)
    assert seen[-1] == ([(4, 6)], 6553.5, False) and set(frame) == {"id", "im", "depth"} and frame["id"] == 2
    s = slam.SlamSession(_config(data=dict(num_frames=8, png_depth_scale=6553.5), png_depth_scale=1000.0), torch.eye(3), torch.eye(4), cam=_Cam())
    gt = np.eye(4, dtype=np.float32)
    frame = s.ingest(0, col, dep, gt_w2c=gt, labels=np.zeros((4, 6), np.uint8))
    assert seen[-1] == ([(4, 6)], 1000.0, True) and set(frame) == {"id", "im", "depth", "gt_w2c", "semantic_label_gt"} and frame["gt_w2c"] is gt
    s.ingest(0, col, dep, png_depth_scale=5000.0)
    assert seen[-1][1] == 5000.0 and len(seen) == 3
