"""The SLAM loop of scripts/hierslam.py as a library: first-frame map, pose seeding, and the per-frame tracking and mapping steps, joined
from the device rows this package already has plus two of its own (row 8): the first-frame map
(include/ext/hsr_map_init.h) and the resample of a frame to the tracking and densification sizes (include/ext/hsr_frame_resample.h).

    initialize_first_timestep(color, depth, intrinsics, w2c, num_frames, scene_radius_depth_ratio, mean_sq_dist_method,
                              gaussian_distribution, num_semantic=None)        scripts/hierslam.py:419-578 with :144-194 and :322-409
    resample_frame(color, depth, sizes)                                        basedataset.py:223-227 (colour, bilinear), :248-252 (depth, nearest)
    initialize_camera_pose(params, curr_time_idx, forward_prop)                :1354-1373
    update_poses(params, sliding_window_kf)                                    :57-70
    matrix_to_quaternion(matrix)                                               what the use_gt_poses branch needs (:1895-1904)
    render_params(params, time_idx, cam, semantic, ...)                        the map from the estimated pose of a frame
    render_view(params, w2c, cam, semantic)                                    the map from a given world-to-camera matrix (eval_nvs,
                                                                               utils/eval_helpers.py:1692-1741; the viz scripts)
    is_keyframe(time_idx, num_frames, keyframe_every, gt_w2c=None)             the rule of :2108-2109
    SlamSession(config, intrinsics, first_frame_w2c, cam, *, keyframe_store="raw")      the body of the frame loop, :1762-2124:
        step(frame)            pose seeding, track_frame, map_frame (every map_every frames), add_keyframe, in the reference's order;
                               the first call (frame id 0) builds the map from the frame and maps it without densification
        track_frame(frame)     :1808-1904      map_frame(frame)     :1927-2083      add_keyframe(frame)     :2107-2124
        tracking_data(frame)   :1792-1799      densify_data(frame)  :1933-1941      {'im', 'depth', 'cam', 'intrinsics'} at that size
        ingest(time_idx, color_u8, depth_raw, ...)      a frame dict for step() from the raw sensor images (hsr_utils.frames), one launch
        replay(out_dir, ...)   the run so far as one picture per step, the map as it stood at each (hsr_utils.replay; the viz scripts)
        save_checkpoint(directory) / load_checkpoint(directory, time_idx, frames=None)      :2128-2133 / :1716-1752 (hsr_utils.checkpoint)

`config` is a dict with the reference's key names (configs/*/*.py): tracking / mapping (num_iters, lrs, loss_weights, sil_thres,
use_sil_for_loss, use_l1, ignore_outlier_depth_loss; tracking: forward_prop, use_gt_poses, use_depth_loss_thres, depth_loss_thres;
mapping: add_new_gaussians, prune_gaussians, pruning_dict, use_gaussian_splatting_densification, densify_dict), map_every,
keyframe_every, mapping_window_size, scene_radius_depth_ratio, mean_sq_dist_method, gaussian_distribution, model.flag_use_embedding.
Three values the reference takes from its dataset object are keys here, since there is no dataset code: data.num_frames (or num_frames),
num_semantic (absent or None: a map without semantics; an int: flat classes; a list: the classes per tree level, K = their sum) and
num_semantic_class (the leaf head's classes, with model.flag_use_embedding = 1).

Tracking and densification may run at sizes of their own (:1543-1563): data.tracking_image_height / _width and
data.densification_image_height / _width (or the same keys at the top level).  Absent keys mean the frame's own size, which is the
camera's (cam.image_height / image_width; desired_image_* is not read); a height without its width, or the reverse, is a KeyError.  The
session then has tracking_cam / tracking_intrinsics and densify_cam / densify_intrinsics (scale_intrinsics by new / old, setup_camera
with the first frame's w2c, :441 and :1698); with the frame's own size they are the very objects cam / intrinsics and nothing is
resampled.  track_frame renders with tracking_cam against the tracking frame (:1792-1799, :1830-1840) and records radii at that size,
as get_loss(tracking_curr_data) does; map_frame hands the silhouette densification the densification frame, camera and intrinsics
(:1933-1951); the first-frame map is built from the densification frame and intrinsics, scene_radius from its depth (:435-456).
Keyframe selection, the mapping iterations, the keyframes and render() stay at the frame's own size (:1966, :1986-2075, :2107-2124).
Both reduced frames come from ONE resample_frame launch per frame (one shared level when the two sizes are equal), cached for the
current frame.  The reference resamples the SENSOR image to each size.  A frame built by ingest() does the same: the frame's own size
and both reduced sizes come from one hsr_frame_ingest launch on the sensor images, the reduced ones travel in the frame as
'tracking_im' / 'tracking_depth' / 'densify_im' / 'densify_depth', and nothing is resampled again.  For a frame NOT built by ingest()
the session resamples the frame it is given: the same thing when that frame is at sensor resolution, not when it was itself resized
(a caller may pass the four tensors above, and they are used in place of the resample).
Semantic sessions take the same route: :1949 passes densify_curr_data to the semantic densification and :480-496 is the first-frame
code, although the reference never constructs the densification dataset for that branch (its own comment at :480: "not run").

A frame is a dict: 'id' (its time index), 'im' [3,H,W] in 0..1, 'depth' [1,H,W], both float32 on the device; optional 'gt_w2c' [4,4]
(relative to frame 0; read by use_gt_poses and by the keyframe rule's validity test), 'semantic_label_gt' [levels (+1 leaf),H,W] and
the four reduced tensors named above.  A frame dict is never modified.

SlamSession(..., keyframe_store="packed") keeps every keyframe as 8-/16-bit codes where those reproduce it bit for bit (a frame from
ingest() at sensor size: 15 instead of 56 bytes per pixel with 5 label planes) and unpacks the members of a mapping window once per
map_frame; save_checkpoint(directory) / load_checkpoint(directory, time_idx) write and resume a run (hsr_utils.checkpoint: the
reference's params{t}.npz and keyframe_time_indices{t}.npy, :2128-2133, plus session{t}.npz with the keyframes in that form, the
bookkeeping, the leaf head's Adam state and the random streams); step() saves when config['save_checkpoints'] is set, every
config['checkpoint_interval'] frames, into config['workdir'] / config['run_name'].

No dataset code, no logging service, no plotting.  There is no CPU path for anything that renders; the pose seeding,
the keyframe rule and the config handling are plain torch / Python and run anywhere.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from diff_gaussian_rasterization import _abi

_lib = _abi.lib

WEIGHT_SEM = (1.0, 5.0)      # scripts/hierslam.py:959, :988
LEAF_FROM_ITER = 14          # :976, :1009


# ---- first-frame map ---------------------------------------------------------------------------------------------------------------
def map_init_frame(color, depth, intrinsics, w2c, scene_radius_depth_ratio, S, capacity=None):
    """hsr_map_init_frame on one RGB-D frame: (count M, means3D, rgb, log_scales [., S], unnorm_rotations, logit_opacities, scene_radius
    [1]); the row tensors hold min(M, capacity) rows (capacity defaults to H*W).  One host read (the count)."""
    if not (torch.is_tensor(depth) and depth.is_cuda and depth.dtype == torch.float32 and color.is_cuda and color.dtype == torch.float32):
        raise RuntimeError("hsr_utils.slam: color and depth must be float32 tensors on a HIP device; there is no CPU path")
    H, W = depth.shape[-2:]
    dev = depth.device
    d = depth.reshape(H, W).contiguous()
    col = color.reshape(-1, H, W).contiguous()
    if col.shape[0] != 3:
        raise RuntimeError("hsr_utils.slam: color must be [3,H,W]")
    K = intrinsics.detach().float().cpu()
    c2w = torch.inverse(w2c.detach().float()).to(dev).contiguous()          # scripts/hierslam.py:167
    cap = H * W if capacity is None else int(capacity)
    o = dict(dtype=torch.float32, device=dev)
    means, rgb, ls = torch.empty((cap, 3), **o), torch.empty((cap, 3), **o), torch.empty((cap, S), **o)
    rots, opac, radius = torch.empty((cap, 4), **o), torch.empty((cap, 1), **o), torch.empty(1, **o)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    sc = torch.empty(int(_lib.hsr_map_init_scratch_bytes(H, W)), dtype=torch.uint8, device=dev)
    _abi.call(_lib.hsr_map_init_frame, "hsr_map_init_frame", dev, H, W, d.data_ptr(), col.data_ptr(), float(K[0, 0]), float(K[1, 1]),
              float(K[0, 2]), float(K[1, 2]), c2w.data_ptr(), float(scene_radius_depth_ratio), cap, int(S), count.data_ptr(),
              means.data_ptr(), rgb.data_ptr(), ls.data_ptr(), rots.data_ptr(), opac.data_ptr(), radius.data_ptr(), sc.data_ptr(), sc.numel())
    M = int(count.item())
    n = min(M, cap)
    return M, means[:n], rgb[:n], ls[:n], rots[:n], opac[:n], radius


RESAMPLE_MAX_SIDE = 16384      # HSR_RESAMPLE_MAX_SIDE


def resample_frame(color, depth, sizes):
    """hsr_frame_resample on one RGB-D frame: `sizes` is a list of one or two (h, w); returns [(color_i [3,h,w], depth_i [1,h,w]), ...].
    Colour bilinear with half-pixel centres and a replicated border, depth nearest with its bits copied, both as cv2.resize does in
    basedataset.py:223-227 and :248-252 (include/ext/hsr_frame_resample.h states every step).  One launch for both levels, no host
    synchronisation.  Non-contiguous input is made contiguous."""
    if not (torch.is_tensor(color) and torch.is_tensor(depth) and color.is_cuda and depth.is_cuda and color.dtype == torch.float32
            and depth.dtype == torch.float32):
        raise RuntimeError("hsr_utils.slam: color and depth must be float32 tensors on a HIP device; there is no CPU path")
    H, W = depth.shape[-2:]
    if color.dim() != 3 or tuple(color.shape) != (3, H, W) or depth.numel() != H * W:
        raise RuntimeError("hsr_utils.slam: color must be [3,H,W] and depth [H,W] or [1,H,W]; got %s and %s" % (tuple(color.shape), tuple(depth.shape)))
    sizes = [(int(h), int(w)) for h, w in sizes]
    if len(sizes) not in (1, 2):
        raise ValueError("hsr_utils.slam: resample_frame takes one or two sizes, not %d" % len(sizes))
    for side in (H, W) + tuple(v for hw in sizes for v in hw):
        if not 1 <= side <= RESAMPLE_MAX_SIDE:
            raise ValueError("hsr_utils.slam: resample_frame sides must be 1..%d; got a frame of %dx%d and sizes %s" % (RESAMPLE_MAX_SIDE, H, W, sizes))
    dev = depth.device
    col, d = color.contiguous(), depth.reshape(H, W).contiguous()
    out = [(torch.empty((3, h, w), dtype=torch.float32, device=dev), torch.empty((1, h, w), dtype=torch.float32, device=dev)) for h, w in sizes]
    (h1, w1), (c1, d1) = (sizes[1], out[1]) if len(sizes) == 2 else ((0, 0), (None, None))
    _abi.call(_lib.hsr_frame_resample, "hsr_frame_resample", dev, H, W, col.data_ptr(), d.data_ptr(), sizes[0][0], sizes[0][1],
              out[0][0].data_ptr(), out[0][1].data_ptr(), h1, w1, None if c1 is None else c1.data_ptr(), None if d1 is None else d1.data_ptr())
    return out


def _scale_columns(gaussian_distribution, semantic):
    if semantic:      # initialize_semantic_params has one column, whatever the config says (:387); so has initialize_new_params_semantic
        return 1
    if gaussian_distribution == "isotropic":
        return 1
    if gaussian_distribution == "anisotropic":
        return 3
    raise ValueError(f"Unknown gaussian_distribution {gaussian_distribution}")


def initialize_first_timestep(color, depth, intrinsics, w2c, num_frames, scene_radius_depth_ratio, mean_sq_dist_method,
                              gaussian_distribution, num_semantic=None):
    """The map and bookkeeping of frame 0 (scripts/hierslam.py:419-578).  Returns (params, variables): nn.Parameters with the keys and
    shapes of initialize_params / initialize_semantic_params (cam_unnorm_rots [1,4,num_frames], cam_trans [1,3,num_frames] included),
    the four bookkeeping vectors zeroed, variables['scene_radius'] set.  num_semantic: None (no 'semantic' key), an int or the list of
    classes per tree level; the semantic rows are torch.rand((N, K)) on the device, as the reference draws them (:376)."""
    if mean_sq_dist_method != "projective":
        raise ValueError(f"Unknown mean_sq_dist_method {mean_sq_dist_method}")
    K_sem = None if num_semantic is None else int(sum(num_semantic) if isinstance(num_semantic, (list, tuple)) else num_semantic)
    S = _scale_columns(gaussian_distribution, K_sem is not None)
    _M, means, rgb, ls, rots, opac, radius = map_init_frame(color, depth, intrinsics, w2c, scene_radius_depth_ratio, S)
    dev = means.device
    num_pts = means.shape[0]
    tensors = {'means3D': means, 'rgb_colors': rgb, 'unnorm_rotations': rots, 'logit_opacities': opac, 'log_scales': ls}
    if K_sem is not None:
        tensors['semantic'] = torch.rand((num_pts, K_sem), device=dev)
    cam_rots = torch.zeros((1, 4, int(num_frames)), dtype=torch.float32, device=dev)
    cam_rots[:, 0, :] = 1.0
    tensors['cam_unnorm_rots'] = cam_rots
    tensors['cam_trans'] = torch.zeros((1, 3, int(num_frames)), dtype=torch.float32, device=dev)
    # clone(): the rows are views of capacity-sized buffers
    params = {k: torch.nn.Parameter(v.float().clone().contiguous().requires_grad_(True)) for k, v in tensors.items()}
    variables = {k: torch.zeros(num_pts, dtype=torch.float32, device=dev)
                 for k in ('max_2D_radius', 'means2D_gradient_accum', 'denom', 'timestep')}
    variables['scene_radius'] = radius[0]
    return params, variables


# ---- poses ---------------------------------------------------------------------------------------------------------------------------
def initialize_camera_pose(params, curr_time_idx, forward_prop):
    """scripts/hierslam.py:1354-1373: frame curr_time_idx starts from the previous pose, or, with forward_prop from the third frame
    on, from the constant-velocity step q1 + (q1 - q2) (both normalised first, the sum normalised again), t1 + (t1 - t2)."""
    with torch.no_grad():
        rots, trans = params['cam_unnorm_rots'], params['cam_trans']
        if curr_time_idx > 1 and forward_prop:
            q1 = F.normalize(rots[..., curr_time_idx - 1].detach())
            q2 = F.normalize(rots[..., curr_time_idx - 2].detach())
            rots[..., curr_time_idx] = F.normalize(q1 + (q1 - q2)).detach()
            t1 = trans[..., curr_time_idx - 1].detach()
            t2 = trans[..., curr_time_idx - 2].detach()
            trans[..., curr_time_idx] = (t1 + (t1 - t2)).detach()
        else:
            rots[..., curr_time_idx] = rots[..., curr_time_idx - 1].detach()
            trans[..., curr_time_idx] = trans[..., curr_time_idx - 1].detach()
    return params


def matrix_to_quaternion(matrix):
    """Rotation matrices [...,3,3] to quaternions [...,4], real part first and non-negative: of the four ways to read a quaternion off
    the matrix, the one whose pivot (4 w^2, 4 x^2, 4 y^2 or 4 z^2) is largest, so that nothing is divided by a small number."""
    if matrix.shape[-2:] != (3, 3):
        raise ValueError(f"Invalid rotation matrix shape {tuple(matrix.shape)}.")
    m = matrix
    m00, m01, m02 = m[..., 0, 0], m[..., 0, 1], m[..., 0, 2]
    m10, m11, m12 = m[..., 1, 0], m[..., 1, 1], m[..., 1, 2]
    m20, m21, m22 = m[..., 2, 0], m[..., 2, 1], m[..., 2, 2]
    pivots = torch.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22], dim=-1)
    rows = torch.stack([
        torch.stack([pivots[..., 0], m21 - m12, m02 - m20, m10 - m01], dim=-1),
        torch.stack([m21 - m12, pivots[..., 1], m10 + m01, m02 + m20], dim=-1),
        torch.stack([m02 - m20, m10 + m01, pivots[..., 2], m21 + m12], dim=-1),
        torch.stack([m10 - m01, m02 + m20, m21 + m12, pivots[..., 3]], dim=-1)], dim=-2)
    best = pivots.argmax(dim=-1)
    q = torch.gather(rows, -2, best[..., None, None].expand(best.shape + (1, 4))).squeeze(-2)
    q = q / (2.0 * torch.sqrt(torch.gather(pivots, -1, best[..., None]).clamp_min(1e-12)))
    return torch.where(q[..., :1] < 0, -q, q)


def frame_w2c(params, time_idx):
    """the estimated world-to-camera of frame time_idx (scripts/hierslam.py:1959-1963, :2112-2116)"""
    from . import densify
    with torch.no_grad():
        return densify._frame_w2c(params, time_idx)


def update_poses(params, sliding_window_kf):
    """scripts/hierslam.py:57-70: refresh every keyframe's est_w2c from the pose parameters"""
    for kf_data in sliding_window_kf:
        kf_data['est_w2c'] = frame_w2c(params, kf_data['id'])


# ---- rules without device work --------------------------------------------------------------------------------------------------------
def is_keyframe(time_idx, num_frames, keyframe_every, gt_w2c=None):
    """scripts/hierslam.py:2108-2109: frame 0, every keyframe_every-th frame, and the second-to-last frame, unless the frame's
    ground-truth pose holds an inf or a NaN (a frame without one counts as valid)."""
    due = time_idx == 0 or (time_idx + 1) % keyframe_every == 0 or time_idx == num_frames - 2
    if not due:
        return False
    if gt_w2c is None:
        return True
    g = torch.as_tensor(gt_w2c)
    return not bool(torch.isinf(g).any()) and not bool(torch.isnan(g).any())


def is_mapping_frame(time_idx, map_every):
    """scripts/hierslam.py:1929"""
    return time_idx == 0 or (time_idx + 1) % map_every == 0


def normalize_config(config):
    """A copy of `config` (the sub-dicts copied too) with the defaults hierslam_main fills in (:1499-1505) and the ones this module
    adds for keys the reference reads from elsewhere; raises KeyError naming the first required key that is missing."""
    cfg = dict(config)
    for section in ('tracking', 'mapping'):
        if section not in cfg:
            raise KeyError("config['%s']" % section)
        cfg[section] = dict(cfg[section])
    for key in ('map_every', 'keyframe_every', 'mapping_window_size'):
        if key not in cfg:
            raise KeyError("config['%s']" % key)
    trk, mp = cfg['tracking'], cfg['mapping']
    if 'use_depth_loss_thres' not in trk:
        trk['use_depth_loss_thres'] = False
        trk['depth_loss_thres'] = 100000
    cfg.setdefault('gaussian_distribution', "isotropic")
    cfg.setdefault('mean_sq_dist_method', "projective")
    cfg.setdefault('scene_radius_depth_ratio', 3)
    for section, name in ((trk, 'tracking'), (mp, 'mapping')):
        for key in ('num_iters', 'lrs', 'loss_weights', 'sil_thres'):
            if key not in section:
                raise KeyError("config['%s']['%s']" % (name, key))
        section.setdefault('use_sil_for_loss', name == 'tracking')
        section.setdefault('use_l1', True)
        section.setdefault('ignore_outlier_depth_loss', False)
        if not section['use_l1']:
            raise ValueError("config['%s']['use_l1'] must be True: the reference defines no other depth loss" % name)
    trk.setdefault('forward_prop', True)
    trk.setdefault('use_gt_poses', False)
    mp.setdefault('add_new_gaussians', True)
    mp.setdefault('prune_gaussians', False)
    mp.setdefault('use_gaussian_splatting_densification', False)
    if mp['prune_gaussians'] and 'pruning_dict' not in mp:
        raise KeyError("config['mapping']['pruning_dict']")
    if mp['use_gaussian_splatting_densification'] and 'densify_dict' not in mp:
        raise KeyError("config['mapping']['densify_dict']")
    cfg['model'] = dict(cfg.get('model') or {})
    cfg['model'].setdefault('flag_use_embedding', 0)
    if 'num_frames' not in cfg:
        if 'num_frames' not in (cfg.get('data') or {}):
            raise KeyError("config['data']['num_frames']")
        cfg['num_frames'] = cfg['data']['num_frames']
    if int(cfg['num_frames']) < 1:
        raise ValueError("num_frames must be the number of frames of the run (there is no dataset to take the length of)")
    data = cfg.get('data') or {}
    for use in ('tracking', 'densification'):      # :1544-1563; absent: the frame's own size (None here; the session knows the frame)
        hk, wk = use + '_image_height', use + '_image_width'
        h, w = (cfg[k] if k in cfg else data.get(k) for k in (hk, wk))
        if (h is None) != (w is None):             # the reference reads the other key of the pair at :1550 / :1560
            raise KeyError("config['data']['%s']" % (wk if w is None else hk))
        if h is not None and (int(h) < 1 or int(w) < 1):
            raise ValueError("%s and %s must be positive, not %r and %r" % (hk, wk, h, w))
        cfg[hk], cfg[wk] = (None, None) if h is None else (int(h), int(w))
    cfg.setdefault('num_semantic', None)
    if cfg['num_semantic'] is not None and cfg['model']['flag_use_embedding'] == 1 and 'num_semantic_class' not in cfg:
        raise KeyError("config['num_semantic_class']")
    if int(cfg['mapping_window_size']) < 2:
        raise ValueError("mapping_window_size counts the last keyframe and the current frame: at least 2")
    cfg.setdefault('save_checkpoints', False)      # :2128-2133
    if cfg['save_checkpoints']:
        for key in ('checkpoint_interval', 'workdir', 'run_name'):
            if key not in cfg:
                raise KeyError("config['%s']" % key)
    return cfg


def render_params(params, time_idx, cam, semantic, gaussians_grad=False, camera_grad=False, retain_means2D=False):
    """(rendervar, im, radius, semantic map | None, depth, final opacity) of the map `params` from the estimated pose of frame time_idx
    with camera `cam`: the semantic rasterizer when `semantic`, else the plain one.  What SlamSession renders with, as a function of
    the parameters alone, so that a finished map (hsr_utils.map_io) can be rendered without a session (evaluate.evaluate_sequence)."""
    from diff_gaussian_rasterization import GaussianRasterizer, GaussianRasterizer_semantic
    from . import slam_helpers as SH
    tg = SH.transform_to_frame(params, time_idx, gaussians_grad=gaussians_grad, camera_grad=camera_grad)
    if semantic:
        rv = SH.transformed_params2rendervar_semantic(params, tg)
        if retain_means2D:
            rv['means2D'].retain_grad()
        im, radius, sem, depth, _median, opac = GaussianRasterizer_semantic(raster_settings=cam)(**rv)
    else:
        rv = SH.transformed_params2rendervar(params, tg)
        if retain_means2D:
            rv['means2D'].retain_grad()
        im, radius, depth, _median, opac, _mask = GaussianRasterizer(raster_settings=cam)(**rv)
        sem = None
    return rv, im, radius, sem, depth, opac


def render_view(params, w2c, cam, semantic):
    """render_params with a world-to-camera matrix in place of time_idx: (rendervar, im, radius, semantic map | None, depth, final
    opacity) of the map `params` seen from `w2c` ([4,4], relative to the first frame like the pose parameters; on the device or the
    host, slam_helpers.transform_to_view) with camera `cam`, under torch.no_grad().  One hsr_view_prep launch in front of the
    rasterizer; nothing of params['cam_unnorm_rots'] / ['cam_trans'] is read, so the view needs no pose column."""
    from diff_gaussian_rasterization import GaussianRasterizer, GaussianRasterizer_semantic
    from . import slam_helpers as SH
    with torch.no_grad():
        tg = SH.transform_to_view(params, w2c)
        if semantic:
            rv = SH.transformed_params2rendervar_semantic(params, tg)
            im, radius, sem, depth, _median, opac = GaussianRasterizer_semantic(raster_settings=cam)(**rv)
        else:
            rv = SH.transformed_params2rendervar(params, tg)
            im, radius, depth, _median, opac, _mask = GaussianRasterizer(raster_settings=cam)(**rv)
            sem = None
    return rv, im, radius, sem, depth, opac


def _param_groups(params, lrs):
    """initialize_optimizer's groups (scripts/hierslam.py:411-417): one named group per parameter"""
    return [{'params': [v], 'name': k, 'lr': lrs[k]} for k, v in params.items()]


# ---- the session ----------------------------------------------------------------------------------------------------------------------
class SlamSession:
    """The state of one run and the per-frame steps (module docstring).  After each call: `params`, `variables`, `keyframe_list`,
    `keyframe_time_indices`, `gt_w2c_all_frames`, `optimizer` (the last one built), `last_window` = (selected_time_idx,
    selected_keyframes) of the last mapping step, `num_tracking_iters` of the last tracked frame."""

    def __init__(self, config, intrinsics, first_frame_w2c, cam, *, keyframe_store="raw"):
        if keyframe_store not in ("raw", "packed"):
            raise ValueError("hsr_utils.slam: keyframe_store must be \"raw\" or \"packed\", not %r" % (keyframe_store,))
        self.keyframe_store = keyframe_store
        self.config = normalize_config(config)
        self.intrinsics, self.first_frame_w2c, self.cam = intrinsics, first_frame_w2c, cam
        self.num_frames = int(self.config['num_frames'])
        ns = self.config['num_semantic']
        self.flag_use_semantic = ns is not None
        self.level_sizes = None if ns is None else ([int(n) for n in ns] if isinstance(ns, (list, tuple)) else None)
        self.num_semantic = None if ns is None else (sum(self.level_sizes) if self.level_sizes is not None else int(ns))
        self.params = self.variables = self.optimizer = None
        self.mlp = self.mlp_optimizer = None
        self.keyframe_list, self.keyframe_time_indices, self.gt_w2c_all_frames = [], [], []
        self.last_window = None
        self.num_tracking_iters = 0
        cfg = self.config
        self.tracking_cam, self.tracking_intrinsics = self._level_camera(cfg['tracking_image_height'], cfg['tracking_image_width'])
        self.densify_cam, self.densify_intrinsics = self._level_camera(cfg['densification_image_height'], cfg['densification_image_width'])
        self._levels = None      # the reduced frames of the current frame: (key, {'tracking': (im, depth), 'densify': (im, depth)}, the frame's tensors)

    # -- tracking and densification resolutions --
    def _level_camera(self, h, w):
        """(camera, intrinsics) of a level of h x w pixels: the session's own objects when that is the frame's size (or no size was
        given), else intrinsics scaled by new / old (basedataset.py:140) and setup_camera on them (scripts/hierslam.py:441, :1698)"""
        if h is None or (h, w) == (self.cam.image_height, self.cam.image_width):
            return self.cam, self.intrinsics
        from .camera import scale_intrinsics, setup_camera
        k = scale_intrinsics(self.intrinsics, h / self.cam.image_height, w / self.cam.image_width)
        k_host = k.detach().cpu().numpy() if torch.is_tensor(k) else k
        w2c = self.first_frame_w2c
        w2c_host = w2c.detach().cpu().numpy() if torch.is_tensor(w2c) else np.asarray(w2c)
        level = setup_camera(w, h, k_host[..., :3, :3], w2c_host, device=self.cam.viewmatrix.device)
        # what is not a matter of size comes from the session's camera; near / far are setup_camera's defaults, as in the reference
        # (a settings tuple does not carry the planes its projection was built with)
        return level._replace(**{f: getattr(self.cam, f) for f in ('bg', 'scale_modifier', 'sh_degree', 'prefiltered', 'debug')}), k

    def _level_data(self, frame):
        """the tracking and densification images and depths of `frame`, computed once per frame (kept until a frame with another id
        or other tensors comes): the caller's own 'tracking_im' / 'tracking_depth' / 'densify_im' / 'densify_depth' where the frame has
        them, the frame's tensors where the level has the frame's size, else ONE resample_frame call for every level still missing
        (one level, shared, when both have the same size)"""
        key = (int(frame['id']), frame['im'].data_ptr(), frame['depth'].data_ptr()) + tuple(
            None if frame.get(k) is None else frame[k].data_ptr() for k in ('tracking_im', 'tracking_depth', 'densify_im', 'densify_depth'))
        if self._levels is not None and self._levels[0] == key:
            return self._levels[1]
        levels, wanted = {}, {}
        for use, cam in (('tracking', self.tracking_cam), ('densify', self.densify_cam)):
            h, w = cam.image_height, cam.image_width
            im, depth = frame.get(use + '_im'), frame.get(use + '_depth')
            if im is not None or depth is not None:
                if im is None or depth is None or tuple(im.shape) != (3, h, w) or tuple(depth.shape) != (1, h, w):
                    raise RuntimeError("hsr_utils.slam: frame %d: '%s_im' must be [3,%d,%d] and '%s_depth' [1,%d,%d]; got %s and %s" % (
                        key[0], use, h, w, use, h, w, None if im is None else tuple(im.shape), None if depth is None else tuple(depth.shape)))
                levels[use] = (im, depth)
            elif cam is self.cam:
                levels[use] = (frame['im'], frame['depth'])
            else:
                wanted.setdefault((h, w), []).append(use)
        if wanted:
            for (_hw, uses), pair in zip(wanted.items(), resample_frame(frame['im'], frame['depth'], list(wanted))):
                for use in uses:
                    levels[use] = pair
        self._levels = (key, levels, (frame['im'], frame['depth']))      # the tensors kept alive: their pointers are the key
        return levels

    def tracking_data(self, frame):
        """what the tracking loop compares against (scripts/hierslam.py:1792-1799): {'im', 'depth', 'cam', 'intrinsics'} at tracking size"""
        im, depth = self._level_data(frame)['tracking']
        return {'im': im, 'depth': depth, 'cam': self.tracking_cam, 'intrinsics': self.tracking_intrinsics}

    def densify_data(self, frame):
        """what the silhouette densification and the first-frame map read (:1933-1941, :435-450), at densification size"""
        im, depth = self._level_data(frame)['densify']
        return {'im': im, 'depth': depth, 'cam': self.densify_cam, 'intrinsics': self.densify_intrinsics}

    def _png_depth_scale(self):
        """config['png_depth_scale'], else config['data']['png_depth_scale'], else None"""
        cfg = self.config
        data = cfg.get('data') or {}
        return cfg['png_depth_scale'] if 'png_depth_scale' in cfg else data.get('png_depth_scale')

    def ingest(self, time_idx, color_u8, depth_raw, gt_w2c=None, labels=None, tree_table=None, png_depth_scale=None, undistort=None,
               leaf_column=False):
        """A frame dict for step() from the raw sensor images (hsr_utils.frames.ingest_frame; basedataset.py:223-227, :248-256,
        replica.py:241-299, scripts/hierslam.py:1777): 'id', 'im' and 'depth' at cam.image_height x cam.image_width, 'gt_w2c' and
        'semantic_label_gt' (int64 [levels + 1, H, W]; tree_table: frames.tree_label_table, None for flat classes) where given, and
        'tracking_im' / 'tracking_depth' / 'densify_im' / 'densify_depth' for every level whose size differs from the frame's — all
        from ONE launch on the sensor image (levels of one size share their tensors), so that step() resamples nothing.
        png_depth_scale defaults to config['data']['png_depth_scale'] (or the same key at the top level); a KeyError without either.
        A depth or label image of another size than the colour image (a ScanNet frame: 968x1296 colour and labels, 480x640 depth), or
        leaf_column=True (tree_table: frames.composed_label_table, whose last column becomes the last label plane: scannet.py:284-339),
        goes through frames.ingest_frame_planes instead: still one launch, each image resampled once per size from its own.
        undistort=(fx, fy, cx, cy, coefficients) of the SENSOR image (a TUM RGB-D frame; coefficients: 4 or 5, OpenCV's order) goes
        through frames.ingest_frame_undistort: the colour image is undistorted inside the same launch, depth and labels are not
        (basedataset.py:306-309), and the frame dict has the same keys.  It does not combine with the planes route: a ValueError."""
        from . import frames
        if png_depth_scale is None:
            png_depth_scale = self._png_depth_scale()
            if png_depth_scale is None:
                raise KeyError("config['data']['png_depth_scale']")
        sizes, uses = [(self.cam.image_height, self.cam.image_width)], {}
        for use, cam in (('tracking', self.tracking_cam), ('densify', self.densify_cam)):
            hw = (cam.image_height, cam.image_width)
            if cam is not self.cam:
                if hw not in sizes:
                    sizes.append(hw)
                uses[use] = sizes.index(hw)
        shape = tuple(getattr(color_u8, 'shape', ()))[:2]      # only shapes that can be read: malformed inputs are ingest_frame's to refuse

        def own_size(image):
            other = tuple(getattr(image, 'shape', ()))
            return len(other) == 2 and other != shape
        if undistort is not None:
            if leaf_column or own_size(depth_raw) or own_size(labels):
                raise ValueError("hsr_utils.slam: ingest: undistort does not combine with the planes route (leaf_column=True, or a depth or "
                                 "label image of another size than the colour image): hsr_frame_ingest_undistort takes one sensor size")
            try:
                fx, fy, cx, cy, coefficients = undistort
            except (TypeError, ValueError):
                raise ValueError("hsr_utils.slam: ingest: undistort must be (fx, fy, cx, cy, coefficients) of the sensor image")
            levels, labels_out = frames.ingest_frame_undistort(color_u8, depth_raw, sizes, png_depth_scale, (fx, fy, cx, cy), coefficients,
                                                               labels=labels, tree_table=tree_table)
        elif leaf_column or own_size(depth_raw) or own_size(labels):
            levels, labels_out = frames.ingest_frame_planes(color_u8, depth_raw, sizes, png_depth_scale, labels=labels, label_table=tree_table,
                                                            leaf_column=leaf_column)
        else:
            levels, labels_out = frames.ingest_frame(color_u8, depth_raw, sizes, png_depth_scale, labels=labels, tree_table=tree_table)
        frame = {'id': int(time_idx), 'im': levels[0][0], 'depth': levels[0][1]}
        if gt_w2c is not None:
            frame['gt_w2c'] = gt_w2c
        if labels_out is not None:
            frame['semantic_label_gt'] = labels_out
        for use, k in uses.items():
            frame[use + '_im'], frame[use + '_depth'] = levels[k]
        return frame

    # -- first frame --
    def initialize(self, frame):
        cfg = self.config
        dd = self.densify_data(frame)      # :435-450: the densification frame and intrinsics; its depth gives scene_radius too (:456)
        self.params, self.variables = initialize_first_timestep(
            dd['im'], dd['depth'], dd['intrinsics'], self.first_frame_w2c, self.num_frames, cfg['scene_radius_depth_ratio'],
            cfg['mean_sq_dist_method'], cfg['gaussian_distribution'], self.num_semantic)
        if self.flag_use_semantic and cfg['model']['flag_use_embedding'] == 1:      # :1755-1758
            dev = self.params['means3D'].device
            self.mlp = torch.nn.Conv2d(self.num_semantic, int(cfg['num_semantic_class']), kernel_size=1).to(dev)
            self.mlp_optimizer = torch.optim.Adam(self.mlp.parameters(), lr=5e-4)
        return self.params, self.variables

    # -- rendering and losses --
    def _render(self, time_idx, gaussians_grad, camera_grad, retain_means2D=False, cam=None):
        return render_params(self.params, time_idx, self.cam if cam is None else cam, self.flag_use_semantic, gaussians_grad, camera_grad,
                             retain_means2D)

    def render(self, time_idx):
        """(im, depth, final opacity, semantic | None) of the map from the estimated pose of frame time_idx, without gradients"""
        with torch.no_grad():
            _rv, im, _radius, sem, depth, opac = self._render(time_idx, False, False)
        return im, depth, opac, sem

    def render_view(self, w2c):
        """(im, depth, final opacity, semantic | None) of the map from the world-to-camera matrix `w2c` ([4,4], relative to the first
        frame), without gradients: render() for a pose that is no frame's (module function render_view)"""
        if self.params is None:
            raise RuntimeError("hsr_utils.slam: render_view before the first frame: there is no map yet")
        _rv, im, _radius, sem, depth, opac = render_view(self.params, w2c, self.cam, self.flag_use_semantic)
        return im, depth, opac, sem

    def _note_seen(self, rv, radius):
        """get_loss*'s bookkeeping (scripts/hierslam.py:1102-1104), without the boolean-mask gathers"""
        v = self.variables
        seen = radius > 0
        v['means2D'] = rv['means2D']
        v['max_2D_radius'] = torch.where(seen, torch.max(radius.to(torch.float32), v['max_2D_radius']), v['max_2D_radius'])
        v['seen'] = seen

    @staticmethod
    def _outlier_mask(gt_depth, depth):
        """the ignore_outlier_depth_loss mask (:910-913) restated in torch: the pixels the fused head (hsr_utils.losses,
        ignore_outlier_depth_loss=True) selects.  The session's losses do not call it; tests/test_gpu_slam_session_outlier.py compares the two."""
        err = torch.abs(gt_depth - depth) * (gt_depth > 0)
        return (err < 10 * err.median()) & (gt_depth > 0) & ~torch.isnan(depth)

    def _tracking_loss(self, frame, im, depth, opac):
        from . import losses as L
        trk = self.config['tracking']
        lw = trk['loss_weights']
        if not trk['ignore_outlier_depth_loss']:
            if trk['use_sil_for_loss']:
                return L.tracking_loss(im, frame['im'], depth, frame['depth'], opac, trk['sil_thres'], True, lw, return_parts=True)
            # :936-937: the colour term runs over every pixel, only the depth term is masked
            d = L.masked_l1(depth, frame['depth'], ((frame['depth'] > 0) & ~torch.isnan(depth)).detach(), "sum")
            c = L.masked_l1(im, frame['im'], None, "sum")
            return L.weighted_sum((d, c), (lw['depth'], lw['im'])), torch.stack((d.detach(), c.detach()))
        # :910-913, :932: the outlier-rejecting mask (restated by _outlier_mask) on both terms, fused: no median sort, no mask tensor
        return L.tracking_loss(im, frame['im'], depth, frame['depth'], opac if trk['use_sil_for_loss'] else None, trk['sil_thres'],
                               trk['use_sil_for_loss'], lw, return_parts=True, ignore_outlier_depth_loss=True)

    def _mapping_loss(self, data, im, sem, depth, it):
        from . import losses as L
        mp = self.config['mapping']
        lw = mp['loss_weights']
        if mp['ignore_outlier_depth_loss']:
            d = L.mapping_depth_loss(depth, data['depth'], ignore_outlier_depth_loss=True)
        else:
            d = L.mapping_depth_loss(depth, data['depth'])
        terms, weights = [d, L.mapping_image_loss(im, data['im'])], [lw['depth'], lw['im']]
        if self.flag_use_semantic:
            lab = data['semantic_label_gt']
            if self.level_sizes is None:
                s = L.cross_entropy_planar(sem, lab)
            elif self.mlp is not None and it >= LEAF_FROM_ITER:
                s = L.semantic_loss_mlp(sem, lab, self.level_sizes, self.mlp, WEIGHT_SEM)
            else:
                H, W = sem.shape[-2:]
                s = L.tree_cross_entropy(sem, lab.reshape(-1, H, W)[:len(self.level_sizes)], self.level_sizes,
                                         [WEIGHT_SEM[0]] * len(self.level_sizes))
            terms.append(s)
            weights.append(lw['sem'])
        return L.weighted_sum(terms, weights)

    # -- (A) tracking --
    def track_frame(self, frame):
        """scripts/hierslam.py:1808-1904 for frame['id'] > 0: the pose of the frame is optimised against the fixed map and the best pose
        seen is kept (on the device, hsr_utils.optim.TrackingCandidate: no host read per iteration); with use_depth_loss_thres the
        iteration budget doubles once when the weighted depth loss is not under depth_loss_thres at its end (one host read there).
        num_iters <= 0 leaves the seeded pose (the reference's loop would not end).  use_gt_poses writes the ground-truth pose."""
        from . import optim
        time_idx = int(frame['id'])
        trk = self.config['tracking']
        self.num_tracking_iters = 0
        if time_idx <= 0:
            return
        params = self.params
        if trk['use_gt_poses']:
            with torch.no_grad():
                rel_w2c = torch.as_tensor(frame['gt_w2c']).to(device=params['cam_trans'].device, dtype=torch.float32)
                params['cam_unnorm_rots'][..., time_idx] = matrix_to_quaternion(rel_w2c[:3, :3].unsqueeze(0).detach())
                params['cam_trans'][..., time_idx] = rel_w2c[:3, 3].detach()
            return
        num_iters = int(trk['num_iters'])
        if num_iters <= 0:
            return
        self.optimizer = optimizer = optim.Adam(_param_groups(params, trk['lrs']))
        candidate = optim.TrackingCandidate(params, time_idx)
        data = self.tracking_data(frame)      # :1792-1799: the frame itself unless tracking has a size of its own
        it, extended = 0, False
        while True:
            rv, im, radius, _sem, depth, opac = self._render(time_idx, gaussians_grad=False, camera_grad=True, cam=data['cam'])
            loss, parts = self._tracking_loss(data, im, depth, opac)
            self._note_seen(rv, radius)
            loss.backward()
            optimizer.step()
            optimizer.zero_grad(set_to_none=True)
            candidate.update(loss)
            it += 1
            if it == num_iters:
                if not trk['use_depth_loss_thres'] or extended:
                    break
                if float(parts[0]) * float(trk['loss_weights']['depth']) < trk['depth_loss_thres']:
                    break
                extended = True
                num_iters = 2 * num_iters
        candidate.restore(params)
        self.num_tracking_iters = it

    # -- (B) mapping --
    def mapping_window(self, frame):
        """scripts/hierslam.py:1957-1974: (selected_time_idx, selected_keyframes) — the overlap selection among keyframe_list[:-1], then
        the last keyframe, then -1 for the current frame"""
        from . import keyframes
        time_idx = int(frame['id'])
        curr_w2c = frame_w2c(self.params, time_idx)
        selected = keyframes.keyframe_selection_overlap(frame['depth'], curr_w2c, self.intrinsics, self.keyframe_list[:-1],
                                                        int(self.config['mapping_window_size']) - 2)
        return keyframes.mapping_window(selected, self.keyframe_list, time_idx)

    def map_frame(self, frame):
        """scripts/hierslam.py:1927-2083: silhouette densification (frames after the first), the mapping window, a fresh optimizer with
        the mapping learning rates, num_iters iterations each on an np.random.randint-chosen member of the window with the mapping loss
        heads; after each backward: prune_gaussians, the optional gradient densification, then the step."""
        from . import densify, optim, slam_external as SE
        cfg, mp = self.config, self.config['mapping']
        time_idx = int(frame['id'])
        if mp['add_new_gaussians'] and time_idx > 0:
            data = dict(self.densify_data(frame), id=time_idx, w2c=self.first_frame_w2c)      # :1933-1941
            if self.flag_use_semantic:
                self.params, self.variables = densify.add_new_gaussians_semantic_newrender(
                    self.params, self.variables, data, mp['sil_thres'], time_idx, cfg['mean_sq_dist_method'], self.num_semantic, flag_use_render=1)
            else:
                self.params, self.variables = densify.add_new_gaussians_newtest(
                    self.params, self.variables, data, mp['sil_thres'], time_idx, cfg['mean_sq_dist_method'], cfg['gaussian_distribution'],
                    flag_use_render=1)
        selected_time_idx, selected_keyframes = self.mapping_window(frame)
        self.last_window = (list(selected_time_idx), list(selected_keyframes))
        self.optimizer = optimizer = optim.Adam(_param_groups(self.params, mp['lrs']), lr=0.0, eps=1e-15)
        gs_densify = bool(mp['use_gaussian_splatting_densification'])
        unpacked = {}      # the packed store: each member of the window unpacked once (at most mapping_window_size - 1 launches), dropped on return
        if self.keyframe_store == "packed":
            from . import checkpoint
            unpacked = {pick: checkpoint.unpack_keyframe(self.keyframe_list[pick]['packed']) for pick in set(selected_keyframes) if pick != -1}
        for it in range(int(mp['num_iters'])):
            pick = selected_keyframes[np.random.randint(0, len(selected_keyframes))]
            if pick == -1:
                data = frame
                iter_time_idx = time_idx
            else:
                kf = self.keyframe_list[pick]
                iter_time_idx = kf['id']
                if pick in unpacked:
                    data = dict(zip(('im', 'depth', 'semantic_label_gt'), unpacked[pick]))
                else:
                    data = {'im': kf['color'], 'depth': kf['depth'], 'semantic_label_gt': kf.get('label_gt')}
            rv, im, radius, sem, depth, _opac = self._render(iter_time_idx, gaussians_grad=True, camera_grad=False, retain_means2D=gs_densify)
            loss = self._mapping_loss(data, im, sem, depth, it)
            self._note_seen(rv, radius)
            loss.backward()
            with torch.no_grad():
                if mp['prune_gaussians']:
                    self.params, self.variables = SE.prune_gaussians(self.params, self.variables, optimizer, it, mp['pruning_dict'])
                if gs_densify:
                    self.params, self.variables = SE.densify(self.params, self.variables, optimizer, it, mp['densify_dict'])
                optimizer.step()
                optimizer.zero_grad(set_to_none=True)
                if self.mlp_optimizer is not None:
                    self.mlp_optimizer.step()
                    self.mlp_optimizer.zero_grad()

    # -- keyframes --
    def add_keyframe(self, frame):
        """scripts/hierslam.py:2107-2124; returns whether the frame became a keyframe"""
        time_idx = int(frame['id'])
        if not is_keyframe(time_idx, self.num_frames, int(self.config['keyframe_every']), frame.get('gt_w2c')):
            return False
        if self.keyframe_store == "packed":
            # 'packed' in place of 'color' / 'depth' / 'label_gt' (hsr_utils.checkpoint): one launch, no host read; the counts of the
            # keyframes before this one have long arrived, and reading them lets go of the planes their codes reproduce
            from . import checkpoint
            for earlier in self.keyframe_list:
                earlier['packed'].resolve()
            labels = frame.get('semantic_label_gt') if self.flag_use_semantic else None
            kf = {'id': time_idx, 'est_w2c': frame_w2c(self.params, time_idx),
                  'packed': checkpoint.pack_keyframe(frame['im'], frame['depth'], labels, self._png_depth_scale()), 'cam': self.cam,
                  'intrinsics': self.intrinsics}
        else:
            kf = {'id': time_idx, 'est_w2c': frame_w2c(self.params, time_idx), 'color': frame['im'], 'depth': frame['depth'], 'cam': self.cam,
                  'intrinsics': self.intrinsics}
            if self.flag_use_semantic:
                kf['label_gt'] = frame.get('semantic_label_gt')
        self.keyframe_list.append(kf)
        self.keyframe_time_indices.append(time_idx)
        return True

    def update_poses(self):
        update_poses(self.params, self.keyframe_list)

    def estimated_w2c(self):
        """the estimated world-to-camera of every frame seen so far, as a list of [4,4] device tensors"""
        return [frame_w2c(self.params, t) for t in range(len(self.gt_w2c_all_frames))]

    def export_map(self, path, **kw):
        """the map as it stands as a PLY file: hsr_utils.map_export.save_map_ply(path, self.params, **kw) — the SH records by default,
        colour="given" | "labels" | "tree" with their arguments for the coloured ones; returns the path"""
        from . import map_export
        if self.params is None:
            raise RuntimeError("hsr_utils.slam: export_map before the first frame: there is no map yet")
        return map_export.save_map_ply(path, self.params, **kw)

    def replay(self, out_dir, **kw):
        """the run so far as one picture per step (and, with cloud=True, one point cloud): hsr_utils.replay.replay_run on the session's
        own params and variables['timestep'], with its intrinsics and frame size; returns the list of steps written"""
        from . import replay
        if self.params is None:
            raise RuntimeError("hsr_utils.slam: replay before the first frame: there is no map yet")
        kw.setdefault('semantic', self.flag_use_semantic)
        kw.setdefault('num_frames', len(self.gt_w2c_all_frames))
        return replay.replay_run(self.params, out_dir, timestep=self.variables['timestep'], intrinsics=self.intrinsics,
                                 width=self.cam.image_width, height=self.cam.image_height, **kw)

    def export_mesh(self, path, **kw):
        """the run so far as a triangle mesh in a PLY file: hsr_utils.mesh.mesh_run on the session's own params — the map rendered with
        the session's camera from every `every`-th estimated pose and fused into a signed distance volume (voxel_size= is required) —
        with its intrinsics, frame size and mapping sil_thres; returns (path, number of vertices, number of faces)"""
        from . import mesh
        if self.params is None:
            raise RuntimeError("hsr_utils.slam: export_mesh before the first frame: there is no map yet")
        kw.setdefault('semantic', self.flag_use_semantic)
        kw.setdefault('num_frames', len(self.gt_w2c_all_frames))
        kw.setdefault('sil_thres', self.config['mapping']['sil_thres'])
        kw.setdefault('cam', self.cam)
        kw.setdefault('first_frame_w2c', self.first_frame_w2c)
        return mesh.mesh_run(self.params, path, intrinsics=self.intrinsics, width=self.cam.image_width, height=self.cam.image_height, **kw)

    def evaluate_mesh(self, gt_ply, **kw):
        """the run so far scored against the ground-truth mesh of its scene: hsr_utils.mesh_eval.evaluate_mesh_run on the session's own
        params — export_mesh's mesh (voxel_size= is required), the ground truth culled to what the estimated poses saw — with the
        session's camera, intrinsics, frame size and mapping sil_thres; returns the dictionary of mesh_metrics and the mesh sizes"""
        from . import mesh_eval
        if self.params is None:
            raise RuntimeError("hsr_utils.slam: evaluate_mesh before the first frame: there is no map yet")
        kw.setdefault('semantic', self.flag_use_semantic)
        kw.setdefault('num_frames', len(self.gt_w2c_all_frames))
        kw.setdefault('sil_thres', self.config['mapping']['sil_thres'])
        kw.setdefault('cam', self.cam)
        kw.setdefault('first_frame_w2c', self.first_frame_w2c)
        return mesh_eval.evaluate_mesh_run(self.params, gt_ply, intrinsics=self.intrinsics, width=self.cam.image_width,
                                           height=self.cam.image_height, **kw)

    def render_mesh(self, out_dir, **kw):
        """pictures of the run's mesh so far, without a window: hsr_utils.mesh_view.render_mesh_run on the session's own params, with its
        intrinsics, frame size and first_frame_w2c, into out_dir.  mesh= is (vertices, faces[, rgb[, labels]]) or the path of a PLY that
        export_mesh wrote; without it export_mesh(out_dir/mesh.ply, voxel_size=...) makes one first (voxel_size= is then required, and
        mesh_every= is its `every`).  Every other keyword is render_mesh_run's (every, orbit, pictures, gt, size, ...).  Returns the
        list of the PNG paths."""
        from . import mesh, mesh_view
        if self.params is None:
            raise RuntimeError("hsr_utils.slam: render_mesh before the first frame: there is no map yet")
        given = kw.pop('mesh', None)
        voxel_size, mesh_every = kw.pop('voxel_size', None), kw.pop('mesh_every', 5)
        if given is None:
            if voxel_size is None:
                raise ValueError("hsr_utils.slam: render_mesh needs mesh= or voxel_size= to make one")
            os.makedirs(out_dir, exist_ok=True)
            given = self.export_mesh(os.path.join(out_dir, "mesh.ply"), voxel_size=voxel_size, every=mesh_every)[0]
        if isinstance(given, (str, os.PathLike)):
            given = mesh.load_mesh_ply(given)
        kw.setdefault('num_frames', len(self.gt_w2c_all_frames))
        kw.setdefault('first_frame_w2c', self.first_frame_w2c)
        return mesh_view.render_mesh_run(self.params, given, out_dir, intrinsics=self.intrinsics, width=self.cam.image_width,
                                         height=self.cam.image_height, **kw)

    def step(self, frame):
        """one pass of the frame loop (scripts/hierslam.py:1762-2124) for frame['id'] = the number of frames stepped so far"""
        time_idx = int(frame['id'])
        if time_idx != len(self.gt_w2c_all_frames):
            raise RuntimeError("hsr_utils.slam: frame %d stepped after %d frames; frames come in order" % (time_idx, len(self.gt_w2c_all_frames)))
        if time_idx >= self.num_frames:
            raise RuntimeError("hsr_utils.slam: frame %d of a run of %d frames" % (time_idx, self.num_frames))
        if time_idx == 0:
            self.initialize(frame)
        self.gt_w2c_all_frames.append(frame.get('gt_w2c'))
        if time_idx > 0:
            initialize_camera_pose(self.params, time_idx, forward_prop=self.config['tracking']['forward_prop'])
        self.track_frame(frame)
        if is_mapping_frame(time_idx, int(self.config['map_every'])):
            self.map_frame(frame)
        self.add_keyframe(frame)
        cfg = self.config
        if cfg['save_checkpoints'] and time_idx % int(cfg['checkpoint_interval']) == 0:      # :2128-2133
            self.save_checkpoint(os.path.join(cfg['workdir'], cfg['run_name']), time_idx)

    # -- checkpoint and resume --
    def save_checkpoint(self, directory, time_idx=None):
        """params{t}.npz and keyframe_time_indices{t}.npy as the reference writes them (:2128-2133) and session{t}.npz with the rest of
        the session, into `directory` (hsr_utils.checkpoint.save_checkpoint); t is the last frame stepped.  Returns the three paths."""
        from . import checkpoint
        return checkpoint.save_checkpoint(self, directory, time_idx)

    def load_checkpoint(self, directory, time_idx, frames=None):
        """Resume this freshly constructed session from the checkpoint of frame time_idx in `directory`
        (hsr_utils.checkpoint.load_checkpoint); returns the id of the frame the next step() takes: time_idx + 1, or time_idx for a
        checkpoint of the reference's own kind (no session{t}.npz; frames(i) must then supply the frame dicts)."""
        from . import checkpoint
        return checkpoint.load_checkpoint(self, directory, time_idx, frames)


__all__ = ["initialize_first_timestep", "initialize_camera_pose", "update_poses", "matrix_to_quaternion", "is_keyframe", "is_mapping_frame",
           "normalize_config", "map_init_frame", "resample_frame", "frame_w2c", "render_params", "render_view", "SlamSession"]
