"""The labels of argmax(softmax(.)) as the library gave them BEFORE the rule moved into csrc/hsr_tree.h, recorded on an MI355X into
tests/golden/tree_labels_parent.npz (tests/golden/make_tree_labels_pin.py; EXPERIMENTS.md §13 names the commit).  The cross-tests of
test_gpu_frame_export.py and test_gpu_map_export.py compare the header's users with one another; this file compares each of them with
the separate copies that went before: hsr_eval_labels_flat / _tree / _leaf, the LOGITS picture of hsr_frame_export in both kernel
variants and the labels of hsr_map_export.  K = 26, levels (3, 5, 8, 6), at 37x53 (an odd pixel count, planes off 16 bytes, a one-pixel
tail of the 4-wide path) and 5x205 (one pixel past whole 256-lane blocks).  The sha256 of every input is recorded and compared first."""
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tree_labels_parent.npz")
SIZES, K = (3, 5, 8, 6), 26
LEVEL_SIZES = list(SIZES) + [99]
SHAPES = ((37, 53), (5, 205))
LEAF_C, MAP_P = 102, 257      # the map: one workgroup of 256 Gaussians and a tail
KEYS = ["%s_%dx%d" % ((n,) + s) for n in ("flat26", "flat22", "tree", "picture", "picture_offset") for s in SHAPES] + ["map_257", "leaf_37x53"]


def frame_logits(shape):
    """float32 [26,H,W]: multiples of 2^-12 in [-8, 8), then the rows of test_logits_equal_the_levels_picture_of_semantic_labels and,
    per level, an image column with one NaN, one with one +inf, one with one -inf, and a column in which a whole level is NaN"""
    g = np.random.default_rng(shape[0] * 1000 + shape[1])
    x = g.integers(-(1 << 15), 1 << 15, size=(K,) + shape).astype(np.float32) * np.float32(2.0 ** -12)
    flat = x.reshape(K, -1)
    flat[1, ::3] = flat[0, ::3] + np.float32(3e-8)                   # within the 1e-6 pre-test: expf and the division decide
    flat[9, 1::3] = np.maximum(flat[8, 1::3], flat[10, 1::3]) + np.float32(5e-7)
    flat[16:22, 2::5] = flat[16, 2::5]                               # the last level all equal
    flat[8:16, 3::11] = np.float32(80.0) * np.arange(8, dtype=np.float32)[:, None]      # differences that underflow expf
    rows, begin = np.arange(shape[0]), np.concatenate([[0], np.cumsum(SIZES)])
    for l, size in enumerate(SIZES):      # columns 4 l .. 4 l + 2: one plane of level l (another one per row) holds NaN, +inf, -inf
        for k, v in enumerate((np.nan, np.inf, -np.inf)):
            x[begin[l] + (rows + k) % size, rows, 4 * l + k] = np.float32(v)
    for y in rows:                        # column 16: the whole of level y % 4 is NaN
        x[begin[y % 4]:begin[y % 4 + 1], y, 16] = np.nan
    x[sum(SIZES):] = np.nan
    return x


def inputs():
    """the frame logits, the tuple colours and the leaf head: sem [26,37,53], weight [102,26], bias [102] of small dyadic numbers, so
    that every leaf logit is exact in fp32 and the duplicated weight rows tie exactly"""
    out = {"logits_%dx%d" % s: frame_logits(s) for s in SHAPES}
    out["tuples"] = np.random.default_rng(4).integers(1, 256, size=(int(np.prod(SIZES)), 3)).astype(np.uint8)      # no black row
    g = np.random.default_rng(102)
    sem = g.integers(-64, 65, size=(K,) + SHAPES[0]).astype(np.float32) * np.float32(2.0 ** -4)
    weight = g.integers(-32, 33, size=(LEAF_C, K)).astype(np.float32) * np.float32(2.0 ** -5)
    bias = g.integers(-16, 17, size=LEAF_C).astype(np.float32) * np.float32(2.0 ** -3)
    for dst, src in ((40, 7), (90, 7), (60, 33), (101, 0), (5, 77)):
        weight[dst], bias[dst] = weight[src], bias[src]
    sem[3, 0, 0], sem[5, 0, 1], sem[7, 0, 2] = np.nan, np.inf, -np.inf
    out["leaf_sem"], out["leaf_weight"], out["leaf_bias"] = sem, weight, bias
    return out


def digests(inp):
    return {"sha256_" + k: np.frombuffer(hashlib.sha256(np.ascontiguousarray(v).tobytes()).digest(), dtype=np.uint8) for k, v in inp.items()}


def labels_of(inp):
    """every recorded array from the library on the device, as uint8"""
    import torch
    from hsr_utils import evaluate
    from hsr_utils.export import export_frame
    from hsr_utils.map_export import gaussian_tree_labels
    u8 = lambda t: t.cpu().numpy().astype(np.uint8)
    out = {}
    tuples = torch.from_numpy(inp["tuples"]).cuda()
    tree_table = torch.zeros(int(np.prod(SIZES)), dtype=torch.int32, device="cuda")
    for shape in SHAPES:
        tag = "%dx%d" % shape
        xd = torch.from_numpy(inp["logits_" + tag]).cuda()
        out["flat26_" + tag] = u8(evaluate.semantic_labels(xd, "flat"))                        # the NaN planes count: label 0
        out["flat22_" + tag] = u8(evaluate.semantic_labels(xd[:sum(SIZES)], "flat"))
        out["tree_" + tag] = u8(evaluate.semantic_labels(xd, "tree", level_sizes=LEVEL_SIZES, tree_table=tree_table)[1])
        out["picture_" + tag] = u8(export_frame(im_semantic=xd, level_sizes=LEVEL_SIZES, tuple_table=tuples)["im_semantic"])
        big = torch.empty(xd.numel() + 1, dtype=torch.float32, device="cuda")      # a view off 16 bytes: the one-pixel-per-lane variant
        big[1:].copy_(xd.reshape(-1))
        assert big[1:].data_ptr() % 16 != 0
        out["picture_offset_" + tag] = u8(export_frame(im_semantic=big[1:].view(xd.shape), level_sizes=LEVEL_SIZES, tuple_table=tuples)["im_semantic"])
    sem = torch.from_numpy(np.ascontiguousarray(inp["logits_37x53"].reshape(K, -1).T[:MAP_P])).cuda()
    out["map_257"] = u8(gaussian_tree_labels(sem, LEVEL_SIZES))
    mlp = (torch.from_numpy(inp["leaf_weight"]).cuda(), torch.from_numpy(inp["leaf_bias"]).cuda())
    out["leaf_37x53"] = u8(evaluate.semantic_labels(torch.from_numpy(inp["leaf_sem"]).cuda(), "leaf", mlp=mlp))
    return out


@pytest.fixture(scope="module")
def recorded():
    want = dict(np.load(GOLDEN))
    inp = inputs()
    for name, digest in digests(inp).items():
        assert np.array_equal(want.pop(name), digest), "the generated input %s is not the recorded one" % name[7:]
    assert sorted(want) == sorted(KEYS)
    return want, labels_of(inp)


@pytest.mark.parametrize("key", KEYS)
def test_labels_are_the_parents(key, recorded):
    want, got = recorded
    assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), "%d labels differ" % int((got[key] != want[key]).sum())
