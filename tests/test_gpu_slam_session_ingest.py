"""GPU suite for SlamSession.ingest: a session fed with raw sensor frames (8-bit interleaved colour, 16-bit depth in units of
1 / 6553.5 m, one raw class-id image) instead of finished tensors.

The sequence is the recipe of tests/test_gpu_slam_session_multires.py (imported for its hidden map, camera path and config): frames at
192x128, tracking and densification at 96x64, K = 4 in a 2 + 2 tree; three frames.  The rendered frames are quantised to uint8 and to
uint16 with scale 6553.5 as the "sensor"; the class id of a pixel is 2 * (level-0 label) + (level-1 label), which the tree table maps
back to the two level labels.

Conditions:
   1. one hsr_frame_ingest launch per frame (the library entry, wrapped) and no resample_frame launch (slam.resample_frame, wrapped);
   2. every keyframe's stored colour and depth are bit-equal to level 0 of ingest_frame on the same sensor images, and the frame's
      'tracking_im' / 'densify_im' share the one reduced level;
   3. every tracking iteration's loss sees [3,64,96] images, every mapping iteration's [3,128,192];
   4. the labels of the frame and of the keyframes are int64 [3,128,192]: the two level planes, then the class id;
   5. the ATE is finite."""
import random

import numpy as np
import pytest
import torch

import test_gpu_slam_session_multires as M

pytestmark = pytest.mark.gpu

W, H, TW, TH = M.W, M.H, M.TW, M.TH
FRAMES = 3
SCALE = 6553.5
TREE = {0: (0, 0), "1": (0, 1), 2: (1, 0), 3: (1, 1)}


@pytest.fixture(scope="module")
def sensor():
    """(cam, intrinsics, [(colour uint8 [H,W,3], depth int16 bits [H,W], class ids uint8 [H,W], gt_w2c)] on the device)"""
    from diff_gaussian_rasterization import GaussianRasterizer_semantic
    from hsr_utils import setup_camera, slam, slam_helpers as SH
    kmat = M._intrinsics()
    cam = setup_camera(W, H, kmat, np.eye(4), device="cuda")
    hidden = {k: v.cuda().contiguous() for k, v in M._hidden_map(kmat).items()}
    rots, trans = M._gt_path()
    hidden["cam_unnorm_rots"], hidden["cam_trans"] = rots.cuda(), trans.cuda()
    raw = []
    with torch.no_grad():
        for t in range(FRAMES):
            rv = SH.transformed_params2rendervar_semantic(hidden, SH.transform_to_frame(hidden, t, False, False))
            im, _radius, sem, depth, _median, opac = GaussianRasterizer_semantic(raster_settings=cam)(**rv)
            assert float(opac.min()) > 0.9
            color_u8 = (im.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
            units = (depth[0] * SCALE).round().clamp(0, 65535).to(torch.int32)
            assert 10000 < int(units.max()) < 32768                # metres of depth, thousands of units
            depth_u16 = units.to(torch.int16)      # the low 16 bits: the sensor's uint16 word
            ids = (2 * sem[:2].argmax(dim=0) + sem[2:4].argmax(dim=0)).to(torch.uint8)
            raw.append((color_u8, depth_u16, ids, slam.frame_w2c(hidden, t)))
    return cam, torch.tensor(kmat, dtype=torch.float32, device="cuda"), raw


@pytest.fixture(scope="module")
def run(sensor):
    from hsr_utils import SlamSession, evaluate, frames, slam, tree_label_table
    cam, intrinsics, raw = sensor
    mp = pytest.MonkeyPatch()
    try:
        launches, resamples = [], []
        real_ingest, real_resample = frames._lib.hsr_frame_ingest, slam.resample_frame
        mp.setattr(frames._lib, "hsr_frame_ingest", lambda *a: launches.append(a) or real_ingest(*a))
        mp.setattr(slam, "resample_frame", lambda *a: resamples.append(a) or real_resample(*a))
        torch.manual_seed(0); np.random.seed(0); random.seed(0)
        cfg = M._config(10)
        cfg["data"]["num_frames"] = FRAMES
        cfg["data"]["png_depth_scale"] = SCALE
        s = SlamSession(cfg, intrinsics, torch.eye(4, device="cuda"), cam)
        table = tree_label_table(TREE, 2, device="cuda")
        log = dict(tracking_shapes=[], mapping_shapes=[], per_frame=[], frames=[])
        tloss_of, mloss_of = s._tracking_loss, s._mapping_loss

        def tracking_loss(data, im, depth, opac):
            log["tracking_shapes"].append((tuple(im.shape), tuple(data["im"].shape), tuple(depth.shape), tuple(data["depth"].shape)))
            return tloss_of(data, im, depth, opac)

        def mapping_loss(data, im, sem, depth, it):
            log["mapping_shapes"].append((tuple(im.shape), tuple(data["im"].shape), tuple(depth.shape), tuple(data["depth"].shape),
                                          data["semantic_label_gt"].dtype, tuple(data["semantic_label_gt"].shape)))
            return mloss_of(data, im, sem, depth, it)
        s._tracking_loss, s._mapping_loss = tracking_loss, mapping_loss
        for t, (color_u8, depth_u16, ids, gt_w2c) in enumerate(raw):
            before = (len(launches), len(resamples))
            frame = s.ingest(t, color_u8, depth_u16, gt_w2c=gt_w2c, labels=ids, tree_table=table)
            s.step(frame)
            log["per_frame"].append((len(launches) - before[0], len(resamples) - before[1]))
            log["frames"].append(frame)
        ate = evaluate.trajectory_ate([r[3] for r in raw], s.estimated_w2c())
        yield s, log, ate, table
    finally:
        mp.undo()


def test_one_ingest_launch_per_frame_and_no_resample(run):
    _s, log, _ate, _table = run
    print("slam_ingest (ingest launches, resample launches) per stepped frame: %s" % log["per_frame"])
    assert log["per_frame"] == [(1, 0)] * FRAMES                                                           # condition 1


def test_frames_and_keyframes_are_the_ingested_sensor_images(run, sensor):
    from hsr_utils import ingest_frame
    s, log, _ate, table = run
    _cam, _k, raw = sensor
    assert [kf["id"] for kf in s.keyframe_list] == [0, 1]
    for frame in log["frames"]:
        assert set(frame) == {"id", "im", "depth", "gt_w2c", "semantic_label_gt", "tracking_im", "tracking_depth", "densify_im", "densify_depth"}
        assert tuple(frame["im"].shape) == (3, H, W) and tuple(frame["depth"].shape) == (1, H, W)
        assert tuple(frame["tracking_im"].shape) == (3, TH, TW) and tuple(frame["tracking_depth"].shape) == (1, TH, TW)
        assert frame["densify_im"] is frame["tracking_im"] and frame["densify_depth"] is frame["tracking_depth"]      # equal sizes are shared
    for kf in s.keyframe_list:                                                                              # condition 2
        color_u8, depth_u16, ids, _gt = raw[kf["id"]]
        levels, labels = ingest_frame(color_u8, depth_u16, [(H, W), (TH, TW)], SCALE, labels=ids, tree_table=table)
        assert torch.equal(kf["color"].view(torch.int32), levels[0][0].view(torch.int32))
        assert torch.equal(kf["depth"].view(torch.int32), levels[0][1].view(torch.int32))
        assert torch.equal(kf["label_gt"], labels)
        frame = log["frames"][kf["id"]]
        assert kf["color"] is frame["im"] and kf["depth"] is frame["depth"]
        assert torch.equal(frame["tracking_im"].view(torch.int32), levels[1][0].view(torch.int32))
        assert torch.equal(frame["tracking_depth"].view(torch.int32), levels[1][1].view(torch.int32))
        # equal sizes: the colour is the sensor's grey level / 255 and the depth the sensor's word / 6553.5, exactly
        want = color_u8.cpu().permute(2, 0, 1).to(torch.float32) / 255      # on the host: IEEE division
        assert torch.equal(kf["color"].cpu(), want)
        units = (depth_u16.cpu().to(torch.int32) & 0xFFFF).to(torch.float64)
        assert torch.equal(kf["depth"][0].cpu(), (units / SCALE).to(torch.float32))


def test_tracking_runs_reduced_and_mapping_at_full_size(run):
    s, log, _ate, _table = run
    small, full = (3, TH, TW), (3, H, W)
    print("slam_ingest loss calls: tracking %d at %s, mapping %d at %s" % (len(log["tracking_shapes"]), small, len(log["mapping_shapes"]), full))
    assert len(log["tracking_shapes"]) == 10 * (FRAMES - 1) and len(log["mapping_shapes"]) == 15 * FRAMES
    assert set(log["tracking_shapes"]) == {(small, small, (1, TH, TW), (1, TH, TW))}                      # condition 3
    assert set(log["mapping_shapes"]) == {(full, full, (1, H, W), (1, H, W), torch.int64, (3, H, W))}     # and 4, as the loss sees them


def test_labels_are_stored_as_int64(run, sensor):
    s, log, _ate, _table = run
    _cam, _k, raw = sensor
    for frame in log["frames"]:                                                                             # condition 4
        lab = frame["semantic_label_gt"]
        assert lab.dtype == torch.int64 and tuple(lab.shape) == (3, H, W) and lab.is_contiguous()
        ids = raw[frame["id"]][2].to(torch.int64)
        assert torch.equal(lab[2], ids) and torch.equal(lab[0], ids // 2) and torch.equal(lab[1], ids % 2)
    for kf in s.keyframe_list:
        assert kf["label_gt"].dtype == torch.int64 and kf["label_gt"] is log["frames"][kf["id"]]["semantic_label_gt"]


def test_the_trajectory_error_is_finite(run):
    _s, _log, ate, _table = run
    print("slam_ingest ATE-RMSE [m] over %d frames fed from 8-bit colour and 16-bit depth: %.6f" % (FRAMES, ate))
    assert np.isfinite(ate)                                                                                 # condition 5
