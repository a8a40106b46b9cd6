"""CPU suite for the keyframe selection: tests/keyframe_ref.py in fp32 on the CPU reproduces the committed outputs of the reference's own
keyframe_selection_overlap (tests/golden/keyframes/*.npz, written by tests/golden/make_keyframe_golden.py), the fixtures meet the
conditions the borderline rule needs, and the prototypes of include/hsr_keyframes.h are exported and bound with the right types (the
one checker of tests/test_abi.py)."""
import glob
import os

import numpy as np
import pytest
import torch

import keyframe_ref as R
from test_abi import check_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "keyframes", "*.npz")))
NAMES = [os.path.basename(p)[:-4] for p in FIXTURES]


def load(path):
    d = np.load(path)
    return d, torch.tensor(d["depth"]), torch.tensor(d["w2c"]), torch.tensor(d["intrinsics"]), torch.tensor(d["est_w2c"])


def test_fixtures_present():
    assert len(FIXTURES) >= 3


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_restatement_reproduces_reference_outputs(path):
    d, depth, w2c, K, poses = load(path)
    torch.manual_seed(int(d["torch_seed"]))
    r = R.overlap(depth, w2c, K, poses, int(d["pixels"]))
    assert np.array_equal(r["pixels"].numpy(), d["sampled_pixels"])
    assert np.array_equal(r["keep"].numpy().astype(np.uint8), d["keep"])
    assert np.array_equal(r["pts"].numpy(), d["pts"])        # the same torch operations as the reference's get_pointcloud
    assert (np.abs(r["counts"] - d["counts"]) <= d["borderline"]).all(), (r["counts"], d["counts"], d["borderline"])
    assert np.array_equal((d["counts"] / np.float32(d["pts"].shape[0])).astype(np.float32), d["percent_inside"])
    torch.manual_seed(int(d["torch_seed"]))
    np.random.seed(int(d["numpy_seed"]))
    got = R.keyframe_selection_overlap(depth, w2c, K, [{'est_w2c': m} for m in poses], int(d["k"]), int(d["pixels"]))
    assert [int(i) for i in got] == d["selected"].tolist()
    # the stored streams are consumed as the reference consumes them: the states afterwards equal those after the draws alone
    t_state, n_state = torch.get_rng_state(), np.random.get_state()[1].copy()
    torch.manual_seed(int(d["torch_seed"]))
    np.random.seed(int(d["numpy_seed"]))
    torch.randint(int((depth[0] > 0).sum()), (int(d["pixels"]),))
    np.random.permutation(np.array(R.selection_order(d["counts"])))
    assert torch.equal(torch.get_rng_state(), t_state) and np.array_equal(np.random.get_state()[1], n_state)


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_float64_decisions_agree_off_the_borderline(path):
    d, depth, w2c, K, poses = load(path)
    H, W = depth.shape[1:]
    sampled = torch.tensor(d["sampled_pixels"].astype(np.int64))
    keep = torch.tensor(d["keep"].astype(bool))
    assert torch.equal(R.keep_by_pixels(sampled, R.back_project(depth, K, w2c, sampled)), keep)
    pts64 = R.back_project(depth, K, w2c, sampled, torch.float64)[keep]
    inside64, border, _u, _v, _m = R.borderline(pts64, poses, K, W, H)
    assert np.array_equal(border.sum(dim=1).numpy(), d["borderline"])
    inside32 = R.project(torch.tensor(d["pts"]), poses, K, W, H)[3]
    assert torch.equal(inside32[~border], inside64[~border])
    assert (np.abs(inside64.sum(dim=1).numpy() - d["counts"]) <= d["borderline"]).all()


def test_fixture_conditions():
    clean, zero = False, False
    for path in FIXTURES:
        d = np.load(path)
        c, b = d["counts"], d["borderline"]
        n_kf, n_pts = len(c), d["pts"].shape[0]
        assert 10 <= n_kf <= 40
        assert b.sum() <= 5e-4 * n_kf * n_pts, path                           # at most 0.05 % of all pairs
        clean |= b.sum() == 0
        zero |= bool(((c == 0) & (b == 0)).any())
        assert not ((c > 0) & (c <= b)).any() and not ((c == 0) & (b > 0)).any(), path   # no count within b of zero
        for i in range(n_kf):
            for j in range(i + 1, n_kf):
                assert (b[i] == 0 and b[j] == 0) or abs(int(c[i]) - int(c[j])) > b[i] + b[j], (path, i, j)
        assert (d["keep"] == 0).any(), path                                    # duplicated draws occur
        assert (d["depth"] == 0).any() and (d["depth"] <= 0).all(axis=2).any(), path   # holes, and rows without a valid pixel
        assert os.path.getsize(path) < 400 * 1024
        pix = d["sampled_pixels"]
        _, inv, cnt = np.unique(pix, axis=0, return_inverse=True, return_counts=True)
        assert np.array_equal(cnt[inv.reshape(-1)] == 1, d["keep"].astype(bool)), path   # removed = drawn more than once
        assert float(d["worst_ref_error_over_m"]) <= 0.25
        assert not set(d["selected"].tolist()) & set(np.nonzero(c == 0)[0].tolist())
        cur = np.abs(d["est_w2c"] - d["w2c"][None]).reshape(n_kf, -1).max(axis=1)
        assert (cur == 0).any(), path                                          # a keyframe at the current pose
    assert clean and zero
    assert any(int(np.load(p)["k"]) > int((np.load(p)["counts"] > 0).sum()) for p in FIXTURES)   # k larger than the candidates


def test_selection_order_is_stable_descending():
    assert R.selection_order([3, 0, 7, 3, 7, 0, 1]) == [2, 4, 0, 3, 6]
    assert R.selection_order([]) == [] and R.selection_order([0, 0]) == []


def test_keyframes_abi_exported_and_bound():
    assert {"hsr_kf_valid_rows", "hsr_kf_sample_points", "hsr_kf_sample_scratch_bytes", "hsr_kf_round_keys",
            "hsr_kf_overlap_counts"} == set(check_header("hsr_keyframes.h"))


def test_argument_validation_without_gpu():
    from hsr_utils import keyframes as KF
    lib = KF._lib
    assert lib.hsr_kf_sample_scratch_bytes(1600) >= 1600 * 12
    assert lib.hsr_kf_valid_rows(0, 8, None, None, None) == -1 and b"kf_valid_rows" in lib.hsr_last_error()
    assert lib.hsr_kf_sample_points(8, 8, None, None, 5000, None, 1.0, 1.0, 0.0, 0.0, *([None] * 6), 0, None) == -1
    assert b"n=5000" in lib.hsr_last_error()
    assert lib.hsr_kf_overlap_counts(-1, None, None, 0, None, None, 8, 8, 20, None, None) == -1
    assert lib.hsr_kf_overlap_counts(0, None, None, 0, None, None, 8, 8, 20, None, None) == 0      # nothing to do, nothing launched
    assert lib.hsr_kf_round_keys(0, None, None, None) == 0


def test_cpu_tensors_are_refused():
    from hsr_utils import keyframes as KF
    depth, eye = torch.ones(1, 8, 8), torch.eye(4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        KF.keyframe_selection_overlap(depth, eye, torch.eye(3), [], 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        KF.overlap_counts(depth, eye, torch.eye(3), [])
    with pytest.raises(RuntimeError, match="no CPU path"):
        KF.round_keys(torch.zeros(4))


def test_keyframe_poses_table_and_mapping_window():
    import hsr_utils
    from hsr_utils import keyframes as KF
    assert hsr_utils.keyframe_selection_overlap is KF.keyframe_selection_overlap and hsr_utils.KeyframePoses is KF.KeyframePoses
    table = KF.KeyframePoses(device="cpu", capacity=2)
    mats = [torch.eye(4) * (i + 1) for i in range(7)]
    for m in mats:
        table.append(m)
    assert len(table) == 7 and table.table().shape == (7, 4, 4) and table.table(3).shape == (3, 4, 4)
    assert torch.equal(table.table(), torch.stack(mats))
    with pytest.raises(RuntimeError):
        table.table(8)
    with pytest.raises(RuntimeError):
        table.append(torch.eye(3))
    # scripts/hierslam.py:1967-1974
    kfl = [{'id': 0}, {'id': 5}, {'id': 10}, {'id': 15}]
    assert KF.mapping_window([np.int64(2), np.int64(0)], kfl, 17) == ([10, 0, 15, 17], [2, 0, 3, -1])
    assert KF.mapping_window([], [], 0) == ([0], [-1])
