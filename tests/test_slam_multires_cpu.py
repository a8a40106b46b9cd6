"""CPU suite for the separate tracking and densification resolutions of hsr_utils.slam: the two float64 restatements of the frame
resample (tests/resample_ref.py) against each other, the prototype of include/ext/hsr_frame_resample.h (its name; tests/test_abi.py
checks that it is exported and bound with the header's types), its argument checks, scale_intrinsics against
datautils.py:73-117, and the four size keys of normalize_config.  Nothing here launches: there is no GPU."""
import copy
import re

import numpy as np
import pytest
import torch

import resample_ref as R
import test_abi

EXT_HEADER = "ext/hsr_frame_resample.h"


@pytest.mark.parametrize("src,dst", R.SIZE_PAIRS, ids=["%dx%d-%dx%d" % (s + d) for s, d in R.SIZE_PAIRS])
def test_the_two_restatements_agree(src, dst):
    """both colours are float64 sums of four terms in [0, 1] (rounding ~1e-16 each): 1e-12; the depths are copies: bit-equal"""
    color, depth = R.make_frame(*src, seed=src[0] + dst[1])
    ct, dt = R.resample_torch(color, depth, dst)
    cs, ds = R.resample_scipy(color, depth, dst)
    assert ct.shape == cs.shape == (3,) + dst and dt.shape == ds.shape == dst and ct.dtype == cs.dtype == torch.float64
    dist = float((ct - cs).abs().max())
    print("resample_ref %dx%d -> %dx%d: torch vs scipy colour distance %.3g" % (src + dst + (dist,)))
    assert dist <= 1e-12
    assert torch.equal(dt.view(torch.int32), ds.view(torch.int32))
    if src == dst:
        assert torch.equal(ct, color.double()) and torch.equal(dt.view(torch.int32), depth.view(torch.int32))
    if src == (16, 16):      # exact 2x: the mean of each 2x2 block, and every second depth
        assert (ct - color.double().reshape(3, 8, 2, 8, 2).mean(dim=(2, 4))).abs().max() <= 1e-15
        assert torch.equal(dt.view(torch.int32), depth[::2, ::2].contiguous().view(torch.int32))


def test_frame_resample_abi_exported_and_bound():
    from diff_gaussian_rasterization import _abi
    protos = test_abi._prototypes([EXT_HEADER])
    assert [s[0] for s in _abi.HEADERS[EXT_HEADER]] == list(protos) == ["hsr_frame_resample"]
    from hsr_utils import slam
    defines = dict(re.findall(r"^#define\s+(HSR_\w+)\s+(\d+)\s*$", test_abi._source(EXT_HEADER), flags=re.M))
    assert slam.RESAMPLE_MAX_SIDE == int(defines["HSR_RESAMPLE_MAX_SIDE"]) == 16384


def test_frame_resample_refuses_before_any_device_work():
    """sizes outside 1..16384 and NULL pointers are an error code and a message, not a launch (the pointers here are all NULL)"""
    from diff_gaussian_rasterization import _abi
    lib = _abi.lib
    null = None

    def call(H, W, H0, W0, H1, W1):
        return lib.hsr_frame_resample(H, W, null, null, H0, W0, null, null, H1, W1, null, null, null)
    for sizes in ((0, 8, 4, 4, 0, 0), (8, 16385, 4, 4, 0, 0), (8, 8, 0, 4, 0, 0), (8, 8, 4, 16385, 0, 0), (8, 8, 4, 4, 16385, 4),
                  (8, 8, 4, 4, 4, 0), (8, 8, 4, 4, -1, 4), (8, 8, -3, 4, 0, 0)):
        assert call(*sizes) == -1 and b"frame_resample: sides" in lib.hsr_last_error(), sizes
    assert call(8, 8, 4, 4, 0, 0) == -1 and b"NULL" in lib.hsr_last_error()      # legal sizes (W1 ignored with H1 == 0), NULL pointers
    assert call(16384, 16384, 16384, 1, 1, 16384) == -1 and b"NULL" in lib.hsr_last_error()


def test_resample_frame_refuses_cpu_tensors_and_bad_arguments():
    from hsr_utils import resample_frame
    color, depth = torch.zeros(3, 4, 6), torch.zeros(1, 4, 6)
    with pytest.raises(RuntimeError, match="no CPU path"):
        resample_frame(color, depth, [(2, 3)])
    with pytest.raises(RuntimeError, match="no CPU path"):
        resample_frame(color.double(), depth, [(2, 3)])


K3 = np.array([[600.0, 0.0, 599.5], [0.0, 600.0, 339.5], [0.0, 0.0, 1.0]])


@pytest.mark.parametrize("kind", ["numpy", "torch"])
@pytest.mark.parametrize("n", [3, 4])
def test_scale_intrinsics(kind, n):
    """datautils.py:73-117: a float32 copy with fx, cx *= w_ratio and fy, cy *= h_ratio; everything else, and the input, untouched"""
    from hsr_utils import scale_intrinsics
    from hsr_utils.camera import scale_intrinsics as from_camera
    assert scale_intrinsics is from_camera
    k = np.eye(n)
    k[:3, :3] = K3
    k = k if kind == "numpy" else torch.tensor(k)
    before = k.copy() if kind == "numpy" else k.clone()
    h_ratio, w_ratio = 18 / 37, 11 / 23
    out = scale_intrinsics(k, h_ratio, w_ratio)
    assert type(out) is type(k) and out.shape == k.shape and out is not k
    assert (out.dtype == np.float32) if kind == "numpy" else (out.dtype == torch.float32)
    assert (k == before).all() and k.dtype == before.dtype                      # the input is left as it was (float64 here)
    got = np.asarray(out, dtype=np.float32) if kind == "numpy" else out.numpy()
    want = np.asarray(before, dtype=np.float64).astype(np.float32)
    for (r, c), ratio in (((0, 0), w_ratio), ((0, 2), w_ratio), ((1, 1), h_ratio), ((1, 2), h_ratio)):
        want[r, c] = np.float32(want[r, c]) * np.float32(ratio)                 # one fp32 product each
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(np.asarray(scale_intrinsics(k, 0.5, 0.5))[:2, :3], np.float32([[300.0, 0.0, 299.75], [0.0, 300.0, 169.75]]))


def test_scale_intrinsics_errors():
    from hsr_utils import scale_intrinsics
    with pytest.raises(TypeError, match="scale_intrinsics: a numpy array or a torch tensor"):
        scale_intrinsics([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]], 0.5, 0.5)
    with pytest.raises(ValueError, match="scale_intrinsics: the last two dimensions must be 3x3 or 4x4"):
        scale_intrinsics(np.eye(2), 0.5, 0.5)
    with pytest.raises(ValueError, match="3x3 or 4x4"):
        scale_intrinsics(torch.eye(3)[:2], 0.5, 0.5)


def _config(**over):
    lrs = dict(means3D=0.0, rgb_colors=0.0, unnorm_rotations=0.0, logit_opacities=0.0, log_scales=0.0, cam_unnorm_rots=4e-4, cam_trans=2e-3)
    cfg = dict(map_every=1, keyframe_every=3, mapping_window_size=4, data=dict(num_frames=8),
               tracking=dict(num_iters=5, lrs=lrs, loss_weights=dict(im=0.5, depth=1.0), sil_thres=0.99),
               mapping=dict(num_iters=5, lrs=lrs, loss_weights=dict(im=0.5, depth=1.0), sil_thres=0.5))
    cfg.update(over)
    return cfg


SIZE_KEYS = ("tracking_image_height", "tracking_image_width", "densification_image_height", "densification_image_width")


def test_config_size_keys():
    from hsr_utils import slam
    out = slam.normalize_config(_config())
    assert all(out[k] is None for k in SIZE_KEYS)                               # absent: the frame's own size, known to the session
    cfg = _config(data=dict(num_frames=8, tracking_image_height=64, tracking_image_width=96, desired_image_height=7, desired_image_width=9))
    frozen = copy.deepcopy(cfg)
    out = slam.normalize_config(cfg)
    assert cfg == frozen
    assert [out[k] for k in SIZE_KEYS] == [64, 96, None, None]                  # from config['data']; desired_image_* is not read
    out = slam.normalize_config(_config(densification_image_height=32, densification_image_width=48))
    assert [out[k] for k in SIZE_KEYS] == [None, None, 32, 48]                  # from the top level
    out = slam.normalize_config(_config(data=dict(num_frames=8, tracking_image_height=64, tracking_image_width=96),
                                        tracking_image_height=16, tracking_image_width=24))
    assert [out[k] for k in SIZE_KEYS] == [16, 24, None, None]                  # the top level wins, as num_frames does
    for use in ("tracking", "densification"):
        for present, missing in (("height", "width"), ("width", "height")):
            for where in ("data", "top"):
                keys = {"%s_image_%s" % (use, present): 64}
                cfg = _config(data=dict(num_frames=8, **keys)) if where == "data" else _config(**keys)
                with pytest.raises(KeyError, match="%s_image_%s" % (use, missing)):
                    slam.normalize_config(cfg)
        for h, w in ((0, 96), (64, 0), (-64, 96), (64, -1)):
            with pytest.raises(ValueError, match="%s_image_height" % use):
                slam.normalize_config(_config(**{use + "_image_height": h, use + "_image_width": w}))


def test_session_without_size_keys_shares_its_camera():
    """no keys: the level cameras and intrinsics are the session's own objects, whatever the camera is (nothing is read from it)"""
    from hsr_utils import slam
    k = torch.eye(3)
    s = slam.SlamSession(_config(), k, torch.eye(4), cam="cam")
    assert s.tracking_cam is s.cam and s.densify_cam is s.cam and s.tracking_intrinsics is k and s.densify_intrinsics is k
