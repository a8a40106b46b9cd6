"""CPU suite for the loop driver (hsr_utils/slam.py): the pose seeding against a float64 restatement of scripts/hierslam.py:1354-1373 written
here, the config handling, the keyframe rule (:2108-2109), the mapping frames (:1929), the assembly order of the mapping window (:1967-1974:
selected, then the last keyframe, then -1 for the current frame), the quaternion of the ground-truth-pose branch, and the prototypes of
include/ext/hsr_map_init.h (their names; tests/test_abi.py checks that they are exported and bound with the header's types).
Nothing here renders: there is no GPU."""
import copy

import numpy as np
import pytest
import torch

import test_abi

EXT_HEADER = "ext/hsr_map_init.h"


def _pose_params(frames, seed, normalised):
    g = torch.Generator().manual_seed(seed)
    q = torch.tensor([1.0, 0.0, 0.0, 0.0]).view(1, 4, 1) + 0.05 * torch.randn(1, 4, frames, generator=g)
    if normalised:
        q = q / q.norm(dim=1, keepdim=True)
    else:
        q = q * (0.5 + 2.0 * torch.rand(1, 1, frames, generator=g))      # stored quaternions are un-normalised: Adam moves them freely
    t = 0.3 * torch.randn(1, 3, frames, generator=g)
    return {"cam_unnorm_rots": torch.nn.Parameter(q.float().contiguous()), "cam_trans": torch.nn.Parameter(t.float().contiguous())}


def _seed_float64(rots, trans, idx, forward_prop):
    """scripts/hierslam.py:1354-1373 in float64: returns the (rotation [4], translation [3]) frame idx starts from"""
    rots, trans = rots.double(), trans.double()

    def unit(q):      # F.normalize: q / max(|q|, 1e-12)
        return q / q.norm().clamp_min(1e-12)
    if idx > 1 and forward_prop:
        q1, q2 = unit(rots[0, :, idx - 1]), unit(rots[0, :, idx - 2])
        t1, t2 = trans[0, :, idx - 1], trans[0, :, idx - 2]
        return unit(q1 + (q1 - q2)), t1 + (t1 - t2)
    return rots[0, :, idx - 1], trans[0, :, idx - 1]


@pytest.mark.parametrize("normalised", [True, False], ids=["unit", "unnormalised"])
@pytest.mark.parametrize("forward_prop", [True, False], ids=["prop", "copy"])
@pytest.mark.parametrize("idx", [1, 2, 5])
def test_initialize_camera_pose_matches_float64(idx, forward_prop, normalised):
    from hsr_utils import initialize_camera_pose
    params = _pose_params(7, 10 * idx + int(forward_prop), normalised)
    before = {k: v.detach().clone() for k, v in params.items()}
    q64, t64 = _seed_float64(before["cam_unnorm_rots"], before["cam_trans"], idx, forward_prop)
    out = initialize_camera_pose(params, idx, forward_prop)
    assert out is params
    q, t = params["cam_unnorm_rots"].detach()[0, :, idx], params["cam_trans"].detach()[0, :, idx]
    if idx > 1 and forward_prop:
        # unit quaternions and translations of size <= ~1.5: a handful of fp32 roundings of values of that size, 6e-8 each
        assert (q.double() - q64).abs().max() <= 5e-7 and (t.double() - t64).abs().max() <= 5e-7
        assert abs(float(q.norm()) - 1.0) <= 2e-7
        assert not torch.equal(q, before["cam_unnorm_rots"][0, :, idx - 1])      # it really propagated
    else:      # no propagation possible (idx 1) or asked for: the previous column, bit for bit, un-normalised as stored
        assert torch.equal(q.double(), q64) and torch.equal(t.double(), t64)
    for k in params:      # every other column is untouched
        keep = [i for i in range(7) if i != idx]
        assert torch.equal(params[k].detach()[..., keep], before[k][..., keep])


def _config(**over):
    lrs_t = dict(means3D=0.0, rgb_colors=0.0, unnorm_rotations=0.0, logit_opacities=0.0, log_scales=0.0, cam_unnorm_rots=4e-4, cam_trans=2e-3)
    lrs_m = dict(means3D=1e-4, rgb_colors=2.5e-3, unnorm_rotations=1e-3, logit_opacities=0.05, log_scales=1e-3, cam_unnorm_rots=0.0, cam_trans=0.0)
    cfg = dict(map_every=1, keyframe_every=3, mapping_window_size=4, data=dict(num_frames=8),
               tracking=dict(num_iters=5, lrs=lrs_t, loss_weights=dict(im=0.5, depth=1.0), sil_thres=0.99),
               mapping=dict(num_iters=5, lrs=lrs_m, loss_weights=dict(im=0.5, depth=1.0), sil_thres=0.5))
    cfg.update(over)
    return cfg


def test_config_keys_and_defaults():
    from hsr_utils import slam
    cfg = _config()
    frozen = copy.deepcopy(cfg)
    out = slam.normalize_config(cfg)
    assert cfg == frozen                                              # the caller's dict is not edited
    assert out["num_frames"] == 8                                     # data.num_frames, where the reference's configs keep it
    assert out["tracking"]["use_depth_loss_thres"] is False and out["tracking"]["depth_loss_thres"] == 100000      # :1499-1501
    assert out["gaussian_distribution"] == "isotropic"                # :1504-1505
    assert out["tracking"]["use_sil_for_loss"] is True and out["mapping"]["use_sil_for_loss"] is False
    assert out["tracking"]["forward_prop"] is True and out["tracking"]["use_gt_poses"] is False
    assert out["mapping"]["add_new_gaussians"] is True and out["mapping"]["prune_gaussians"] is False
    assert out["model"]["flag_use_embedding"] == 0 and out["num_semantic"] is None
    assert slam.normalize_config(_config(num_frames=5))["num_frames"] == 5      # a top-level num_frames wins
    for drop, named in ((("tracking",), "tracking"), (("mapping", "lrs"), "lrs"), (("map_every",), "map_every"),
                        (("keyframe_every",), "keyframe_every"), (("mapping_window_size",), "mapping_window_size"),
                        (("data",), "num_frames"), (("tracking", "sil_thres"), "sil_thres")):
        bad = copy.deepcopy(_config())
        holder = bad
        for k in drop[:-1]:
            holder = holder[k]
        del holder[drop[-1]]
        with pytest.raises(KeyError, match=named):
            slam.normalize_config(bad)
    with pytest.raises(KeyError, match="pruning_dict"):
        slam.normalize_config(_config(mapping=dict(_config()["mapping"], prune_gaussians=True)))
    with pytest.raises(KeyError, match="num_semantic_class"):
        slam.normalize_config(_config(num_semantic=[2, 2], model=dict(flag_use_embedding=1)))
    with pytest.raises(ValueError, match="num_frames"):
        slam.normalize_config(_config(data=dict(num_frames=-1)))
    with pytest.raises(ValueError, match="use_l1"):
        slam.normalize_config(_config(tracking=dict(_config()["tracking"], use_l1=False)))
    with pytest.raises(ValueError, match="mapping_window_size"):
        slam.normalize_config(_config(mapping_window_size=1))
    s = slam.SlamSession(_config(num_semantic=[2, 3]), torch.eye(3), torch.eye(4), cam=None)
    assert s.flag_use_semantic and s.num_semantic == 5 and s.level_sizes == [2, 3] and s.num_frames == 8
    s = slam.SlamSession(_config(num_semantic=7), torch.eye(3), torch.eye(4), cam=None)
    assert s.flag_use_semantic and s.num_semantic == 7 and s.level_sizes is None
    assert not slam.SlamSession(_config(), torch.eye(3), torch.eye(4), cam=None).flag_use_semantic


def test_first_timestep_rejects_unknown_methods():
    from hsr_utils import initialize_first_timestep
    z = torch.zeros(1, 2, 2)
    with pytest.raises(ValueError, match="Unknown mean_sq_dist_method nearest"):
        initialize_first_timestep(torch.zeros(3, 2, 2), z, torch.eye(3), torch.eye(4), 4, 3, "nearest", "isotropic")
    with pytest.raises(ValueError, match="Unknown gaussian_distribution round"):
        initialize_first_timestep(torch.zeros(3, 2, 2), z, torch.eye(3), torch.eye(4), 4, 3, "projective", "round")
    with pytest.raises(RuntimeError, match="no CPU path"):
        initialize_first_timestep(torch.zeros(3, 2, 2), z, torch.eye(3), torch.eye(4), 4, 3, "projective", "isotropic")


def test_keyframe_and_mapping_rules():
    from hsr_utils import slam
    n, every = 8, 3
    ids = [t for t in range(n) if slam.is_keyframe(t, n, every)]
    assert ids == [0, 2, 5, 6]                                        # frame 0, (t + 1) % 3 == 0, and the second-to-last frame
    assert [t for t in range(6) if slam.is_keyframe(t, 6, 2)] == [0, 1, 3, 4, 5]
    good = torch.eye(4)
    assert slam.is_keyframe(2, n, every, good)
    for poison in (float("nan"), float("inf"), -float("inf")):
        bad = good.clone()
        bad[1, 3] = poison
        assert not slam.is_keyframe(2, n, every, bad)
    assert not slam.is_keyframe(3, n, every, good)
    assert [t for t in range(8) if slam.is_mapping_frame(t, 3)] == [0, 2, 5]
    assert [t for t in range(4) if slam.is_mapping_frame(t, 1)] == [0, 1, 2, 3]


def _cpu_session(num_frames=8, **over):
    from hsr_utils import slam
    s = slam.SlamSession(_config(**over), torch.eye(3), torch.eye(4), cam="cam")
    s.num_frames = num_frames
    s.params = _pose_params(num_frames, 3, normalised=False)
    return s


def test_add_keyframe_bookkeeping():
    from hsr_utils import slam
    s = _cpu_session()
    frames = [{"id": t, "im": torch.full((3, 2, 2), float(t)), "depth": torch.ones(1, 2, 2), "gt_w2c": torch.eye(4)} for t in range(8)]
    frames[5]["gt_w2c"] = torch.full((4, 4), float("nan"))
    added = [s.add_keyframe(f) for f in frames]
    assert added == [True, False, True, False, False, False, True, False]
    assert s.keyframe_time_indices == [0, 2, 6] == [kf["id"] for kf in s.keyframe_list]
    kf = s.keyframe_list[1]
    assert set(kf) == {"id", "est_w2c", "color", "depth", "cam", "intrinsics"} and kf["color"] is frames[2]["im"] and kf["cam"] == "cam"
    # est_w2c is the pose parameters' matrix: rotation of the normalised quaternion, translation as stored
    q = torch.nn.functional.normalize(s.params["cam_unnorm_rots"].detach()[0, :, 2].double(), dim=0)
    r, x, y, z = q
    rot = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)]),
                       torch.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)]),
                       torch.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)])])
    assert (kf["est_w2c"][:3, :3].double() - rot).abs().max() <= 1e-6
    assert torch.equal(kf["est_w2c"][:3, 3], s.params["cam_trans"].detach()[0, :, 2]) and torch.equal(kf["est_w2c"][3], torch.tensor([0.0, 0, 0, 1]))
    # update_poses follows the parameters
    with torch.no_grad():
        s.params["cam_trans"][0, :, 2] += 1.0
    s.update_poses()
    assert torch.equal(s.keyframe_list[1]["est_w2c"][:3, 3], s.params["cam_trans"].detach()[0, :, 2])
    # the round trip of the ground-truth-pose branch: matrix -> quaternion -> the same rotation
    q2 = slam.matrix_to_quaternion(rot[None])[0]
    assert (q2 - q * torch.sign(q[0])).abs().max() <= 1e-12 and q2[0] >= 0
    semantic = slam.SlamSession(_config(num_semantic=[2, 2]), torch.eye(3), torch.eye(4), cam=None)
    semantic.params = s.params
    semantic.add_keyframe(dict(frames[0], semantic_label_gt="labels"))
    assert semantic.keyframe_list[0]["label_gt"] == "labels"


@pytest.mark.parametrize("n_keyframes,selected", [(0, []), (1, []), (4, [2, 0]), (5, [1, 3])])
def test_mapping_window_order(monkeypatch, n_keyframes, selected):
    """selected keyframes (among all but the last one), then the last keyframe, then -1 for the current frame; the time indices alongside"""
    from hsr_utils import keyframes
    s = _cpu_session(num_frames=20, mapping_window_size=4)
    s.keyframe_list = [{"id": 3 * i, "est_w2c": torch.eye(4)} for i in range(n_keyframes)]
    seen = {}

    def fake_selection(gt_depth, w2c, intrinsics, keyframe_list, k, **kw):
        seen.update(depth=gt_depth, n=len(keyframe_list), k=k, ids=[kf["id"] for kf in keyframe_list], w2c=w2c)
        return [np.int64(i) for i in selected]
    monkeypatch.setattr(keyframes, "keyframe_selection_overlap", fake_selection)
    frame = {"id": 17, "depth": torch.ones(1, 2, 2), "im": torch.zeros(3, 2, 2)}
    time_idx, window = s.mapping_window(frame)
    assert seen["n"] == max(0, n_keyframes - 1) and seen["ids"] == [3 * i for i in range(max(0, n_keyframes - 1))]      # keyframe_list[:-1]
    assert seen["k"] == 2 and seen["depth"] is frame["depth"]                                                            # window size - 2
    assert torch.equal(seen["w2c"][:3, 3], s.params["cam_trans"].detach()[0, :, 17])                                     # the current estimate
    last = [n_keyframes - 1] if n_keyframes else []
    assert [int(i) for i in window] == selected + last + [-1]
    assert time_idx == [3 * i for i in selected] + [3 * i for i in last] + [17]


def test_step_refuses_frames_out_of_order():
    s = _cpu_session()
    with pytest.raises(RuntimeError, match="frames come in order"):
        s.step({"id": 2})
    s.gt_w2c_all_frames = [None] * 8
    with pytest.raises(RuntimeError, match="of a run of 8 frames"):
        s.step({"id": 8})


def test_map_init_abi_exported_and_bound():
    from diff_gaussian_rasterization import _abi
    protos = test_abi._prototypes([EXT_HEADER])
    assert [s[0] for s in _abi.HEADERS[EXT_HEADER]] == list(protos) == ["hsr_map_init_scratch_bytes", "hsr_map_init_frame"]


def test_map_init_host_only_entry_points():
    """sizes are answered and illegal arguments refused before any device work"""
    from diff_gaussian_rasterization import _abi
    lib = _abi.lib
    assert lib.hsr_map_init_scratch_bytes(0, 5) > 0
    small, large = lib.hsr_map_init_scratch_bytes(64, 48), lib.hsr_map_init_scratch_bytes(680, 1200)
    assert 2 * 4 * (64 * 48 // 256) <= small < large and large >= 2 * 4 * (680 * 1200 // 256)      # a count and a maximum per 256 pixels
    null = None
    args = (null, null, 1.0, 1.0, 0.0, 0.0, null, 3.0, 0, 1, *([null] * 7), null, 0, null)
    assert lib.hsr_map_init_frame(0, 8, *args) == -1 and b"map_init_frame" in lib.hsr_last_error()
    assert lib.hsr_map_init_frame(8, 8, *args) == -1 and b"NULL" in lib.hsr_last_error()
