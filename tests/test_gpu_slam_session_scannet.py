"""GPU suite for a session fed from a ScanNet-layout directory: colour and class ids at a sensor size of their own, depth at the frame's
size, read back through hsr_utils.ScanNetSequence and ingested with SlamSession.ingest(..., leaf_column=True).

The sequence is the recipe of tests/test_gpu_slam_session_ingest.py (tests/test_gpu_slam_session_multires.py, imported for its hidden
map, camera path and config): frames at 192x128, tracking and densification at 96x64, K = 4 in a 2 + 2 tree; three frames.  The
"sensor" colour and class-id images are rendered by a second camera at 389x259 (ScanNet's 2.02 ratio, both sides odd) whose intrinsics
are scale_intrinsics of the frame's; the depth is rendered at the frame's 192x128.  A pixel's leaf class is 2 * (level-0 label) +
(level-1 label); the label image holds RAW ids beyond 8 bits, which a class mapping takes to the leaf and the tree to the two levels.
The images are written as color/*.jpg, depth/*.png (millimetres), label-filt/*.png (16 bit) and pose/*.txt (camera-to-world).

Conditions:
   1. one hsr_frame_ingest_planes call per frame, no hsr_frame_ingest call and no resample_frame call (all three wrapped);
   2. every keyframe's colour, depth and label planes, and the frames' reduced level, are bit-equal to the restatement
      (tests/ingest_planes_ref.py) on the decoded files;
   3. every tracking iteration's loss sees [3,64,96] images, every mapping iteration's [3,128,192] with int64 [3,128,192] labels;
   4. the last label plane holds the mapped leaf class, not the raw id;
   5. the row counts of parameters, Adam moments and bookkeeping agree after every step, and the ATE is finite."""
import random

import numpy as np
import pytest
import torch

import ingest_planes_ref as P
import test_gpu_slam_session_multires as M

pytestmark = pytest.mark.gpu

W, H, TW, TH = M.W, M.H, M.TW, M.TH
SENSOR_W, SENSOR_H = 389, 259
FRAMES = 3
SCALE = 1000.0
RAW_OF_LEAF = (7, 300, 41, 1200)                                   # the raw id the "sensor" writes for leaf 0..3
CLASSES = {7: 0, 300: 1, "41": 2, 1200: 3, 2: 1}                   # raw id -> leaf; 2 -> 1 never occurs in the images
TREE = {0: (0, 0), "1": (0, 1), 2: (1, 0), 3: (1, 1)}              # leaf -> the two level labels


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.int32)


@pytest.fixture(scope="module")
def scannet(tmp_path_factory):
    """(frame cam, frame intrinsics, ScanNetSequence over the directory this fixture renders and writes, the gt w2c of the hidden path)"""
    from PIL import Image
    from diff_gaussian_rasterization import GaussianRasterizer_semantic
    from hsr_utils import ScanNetSequence, scale_intrinsics, setup_camera, slam, slam_helpers as SH
    kmat = np.asarray(M._intrinsics(), dtype=np.float64)
    cam = setup_camera(W, H, kmat, np.eye(4), device="cuda")
    sensor_cam = setup_camera(SENSOR_W, SENSOR_H, scale_intrinsics(kmat, SENSOR_H / H, SENSOR_W / W), np.eye(4), device="cuda")
    hidden = {k: v.cuda().contiguous() for k, v in M._hidden_map(M._intrinsics()).items()}
    rots, trans = M._gt_path()
    hidden["cam_unnorm_rots"], hidden["cam_trans"] = rots.cuda(), trans.cuda()
    base = tmp_path_factory.mktemp("scannet_session")
    seq_dir = base / "scene0000_00"
    for sub in ("color", "depth", "pose", "label-filt"):
        (seq_dir / sub).mkdir(parents=True)
    raw_of_leaf = torch.tensor(RAW_OF_LEAF, dtype=torch.int64, device="cuda")
    gts = []
    with torch.no_grad():
        for t in range(FRAMES):
            rv = SH.transformed_params2rendervar_semantic(hidden, SH.transform_to_frame(hidden, t, False, False))
            im, _radius, sem, _depth, _median, _opac = GaussianRasterizer_semantic(raster_settings=sensor_cam)(**rv)
            _im, _radius, _sem, depth, _median, opac = GaussianRasterizer_semantic(raster_settings=cam)(**rv)
            assert float(opac.min()) > 0.9
            assert tuple(im.shape) == (3, SENSOR_H, SENSOR_W) and tuple(depth.shape) == (1, H, W)
            color_u8 = (im.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().cpu().numpy()
            units = (depth[0] * SCALE).round().clamp(0, 65535).to(torch.int32).cpu().numpy().astype(np.uint16)
            assert 1500 < int(units.max()) < 6000                  # metres of depth, thousands of millimetres
            leaf = 2 * sem[:2].argmax(dim=0) + sem[2:4].argmax(dim=0)
            raw_ids = raw_of_leaf[leaf].cpu().numpy().astype(np.uint16)
            name = str(9 + t)                                      # 9, 10, 11: numeric order, not the characters'
            Image.fromarray(color_u8).save(seq_dir / "color" / (name + ".jpg"), quality=95)
            Image.fromarray(units).save(seq_dir / "depth" / (name + ".png"))
            Image.fromarray(raw_ids).save(seq_dir / "label-filt" / (name + ".png"))
            w2c = slam.frame_w2c(hidden, t).detach().cpu().numpy().astype(np.float64)
            gts.append(w2c)
            with open(seq_dir / "pose" / (name + ".txt"), "w") as f:
                for row in np.linalg.inv(w2c):
                    f.write(" ".join(repr(float(v)) for v in row) + "\n")
    return cam, torch.tensor(M._intrinsics(), dtype=torch.float32, device="cuda"), ScanNetSequence(str(base), "scene0000_00"), gts


@pytest.fixture(scope="module")
def run(scannet):
    from hsr_utils import SlamSession, composed_label_table, evaluate, frames, slam
    cam, intrinsics, seq, _gts = scannet
    mp = pytest.MonkeyPatch()
    try:
        planes, launches, resamples = [], [], []
        real_planes, real_ingest, real_resample = frames._lib.hsr_frame_ingest_planes, frames._lib.hsr_frame_ingest, slam.resample_frame
        mp.setattr(frames._lib, "hsr_frame_ingest_planes", lambda *a: planes.append(a) or real_planes(*a))
        mp.setattr(frames._lib, "hsr_frame_ingest", lambda *a: launches.append(a) or real_ingest(*a))
        mp.setattr(slam, "resample_frame", lambda *a: resamples.append(a) or real_resample(*a))
        torch.manual_seed(0); np.random.seed(0); random.seed(0)
        cfg = M._config(10)
        cfg["data"]["num_frames"] = FRAMES
        cfg["data"]["png_depth_scale"] = SCALE
        s = SlamSession(cfg, intrinsics, torch.eye(4, device="cuda"), cam)
        table = composed_label_table(CLASSES, TREE, 2, device="cuda")
        log = dict(tracking_shapes=[], mapping_shapes=[], per_frame=[], frames=[], raw=[], rows=[], counts=[])
        tloss_of, mloss_of = s._tracking_loss, s._mapping_loss

        def tracking_loss(data, im, depth, opac):
            log["tracking_shapes"].append((tuple(im.shape), tuple(data["im"].shape), tuple(depth.shape), tuple(data["depth"].shape)))
            return tloss_of(data, im, depth, opac)

        def mapping_loss(data, im, sem, depth, it):
            log["mapping_shapes"].append((tuple(im.shape), tuple(data["im"].shape), tuple(depth.shape), tuple(data["depth"].shape),
                                          data["semantic_label_gt"].dtype, tuple(data["semantic_label_gt"].shape)))
            return mloss_of(data, im, sem, depth, it)
        s._tracking_loss, s._mapping_loss = tracking_loss, mapping_loss
        for t in range(len(seq)):
            color_u8, depth_u16, ids, gt_w2c = seq[t]
            before = (len(planes), len(launches), len(resamples))
            frame = s.ingest(t, color_u8, depth_u16, gt_w2c=gt_w2c, labels=ids, tree_table=table, leaf_column=True)
            s.step(frame)
            log["per_frame"].append((len(planes) - before[0], len(launches) - before[1], len(resamples) - before[2]))
            log["frames"].append(frame)
            log["raw"].append((color_u8, depth_u16, ids, gt_w2c))
            log["counts"].append(int(s.params["means3D"].shape[0]))
            log["rows"].append(M._row_counts(s))
        ate = evaluate.trajectory_ate([r[3] for r in log["raw"]], s.estimated_w2c())
        yield s, log, ate, table
    finally:
        mp.undo()


def test_the_sequence_is_what_the_session_should_see(scannet):
    _cam, _k, seq, gts = scannet
    assert len(seq) == FRAMES and [p.rsplit("/", 1)[-1] for p in seq.color_paths] == ["9.jpg", "10.jpg", "11.jpg"]
    for t in range(FRAMES):
        color, depth, ids, gt_w2c = seq[t]
        assert color.dtype == np.uint8 and color.shape == (SENSOR_H, SENSOR_W, 3) and depth.dtype == np.uint16 and depth.shape == (H, W)
        assert ids.dtype == np.int32 and ids.shape == (SENSOR_H, SENSOR_W) and set(np.unique(ids).tolist()) <= set(RAW_OF_LEAF) and len(np.unique(ids)) == 4
        assert np.abs(gt_w2c - gts[t] @ np.linalg.inv(gts[0])).max() <= 1e-6      # relative to the first frame, whose pose is the identity


def test_one_planes_call_per_frame_and_nothing_else(run):
    _s, log, _ate, _table = run
    print("slam_scannet (planes calls, ingest calls, resample calls) per stepped frame: %s" % log["per_frame"])
    assert log["per_frame"] == [(1, 0, 0)] * FRAMES                                                         # condition 1


def test_keyframes_are_the_restatement_on_the_decoded_files(run):
    s, log, _ate, table = run
    assert [kf["id"] for kf in s.keyframe_list] == [0, 1]
    for frame in log["frames"]:
        assert set(frame) == {"id", "im", "depth", "gt_w2c", "semantic_label_gt", "tracking_im", "tracking_depth", "densify_im", "densify_depth"}
        assert tuple(frame["im"].shape) == (3, H, W) and tuple(frame["depth"].shape) == (1, H, W)
        assert tuple(frame["tracking_im"].shape) == (3, TH, TW) and tuple(frame["tracking_depth"].shape) == (1, TH, TW)
        assert frame["densify_im"] is frame["tracking_im"] and frame["densify_depth"] is frame["tracking_depth"]      # equal sizes are shared
    for kf in s.keyframe_list:                                                                              # condition 2
        color_u8, depth_u16, ids, _gt = log["raw"][kf["id"]]
        (full, small), labels = P.frame(color_u8, depth_u16, [(H, W), (TH, TW)], SCALE, ids, table.cpu().numpy(), True)
        frame = log["frames"][kf["id"]]
        assert kf["color"] is frame["im"] and kf["depth"] is frame["depth"] and kf["label_gt"] is frame["semantic_label_gt"]
        assert np.array_equal(_bits(kf["color"]), full[0].view(np.int32)) and np.array_equal(_bits(kf["depth"][0]), full[1].view(np.int32))
        assert np.array_equal(kf["label_gt"].cpu().numpy(), labels)
        assert np.array_equal(_bits(frame["tracking_im"]), small[0].view(np.int32))
        assert np.array_equal(_bits(frame["tracking_depth"][0]), small[1].view(np.int32))
        # the depth has the frame's size: the sensor's word / 1000, exactly
        assert torch.equal(kf["depth"][0].cpu(), torch.from_numpy((depth_u16.astype(np.float64) / SCALE).astype(np.float32)))


def test_tracking_runs_reduced_and_mapping_at_full_size(run):
    _s, log, _ate, _table = run
    small, full = (3, TH, TW), (3, H, W)
    print("slam_scannet loss calls: tracking %d at %s, mapping %d at %s" % (len(log["tracking_shapes"]), small, len(log["mapping_shapes"]), full))
    assert len(log["tracking_shapes"]) == 10 * (FRAMES - 1) and len(log["mapping_shapes"]) == 15 * FRAMES
    assert set(log["tracking_shapes"]) == {(small, small, (1, TH, TW), (1, TH, TW))}                      # condition 3
    assert set(log["mapping_shapes"]) == {(full, full, (1, H, W), (1, H, W), torch.int64, (3, H, W))}


def test_the_last_plane_is_the_mapped_class(run):
    _s, log, _ate, _table = run
    for frame, (_c, _d, ids, _gt) in zip(log["frames"], log["raw"]):                                        # condition 4
        lab = frame["semantic_label_gt"]
        assert lab.dtype == torch.int64 and tuple(lab.shape) == (3, H, W) and lab.is_contiguous()
        leaf = lab[2].cpu().numpy()
        assert set(np.unique(leaf).tolist()) == {0, 1, 2, 3}                                             # leaves, none of 7, 300, 41, 1200
        ys, xs = (np.arange(H) * SENSOR_H) // H, (np.arange(W) * SENSOR_W) // W
        raw = ids[ys[:, None], xs[None, :]]
        assert np.array_equal(np.asarray(RAW_OF_LEAF)[leaf], raw)
        assert torch.equal(lab[0], lab[2] // 2) and torch.equal(lab[1], lab[2] % 2)


def test_row_counts_agree_and_the_trajectory_error_is_finite(run):
    _s, log, ate, _table = run
    print("slam_scannet Gaussians after each step: %s; ATE-RMSE [m] over %d frames: %.6f" % (log["counts"], FRAMES, ate))
    for t, rows in enumerate(log["rows"]):                                                                  # condition 5
        assert set(rows.values()) == {log["counts"][t]}, (t, rows)
        assert any(k.startswith("exp_avg_sq/") for k in rows)
    assert np.isfinite(ate)
