"""The SLAM loop of scripts/hierslam.py as a library: first-frame map, pose seeding, and the per-frame tracking and mapping steps, joined
from the device rows this package already has plus one new one, the first-frame map (row 8, include/ext/hsr_map_init.h).

    initialize_first_timestep(color, depth, intrinsics, w2c, num_frames, scene_radius_depth_ratio, mean_sq_dist_method,
                              gaussian_distribution, num_semantic=None)        scripts/hierslam.py:419-578 with :144-194 and :322-409
    initialize_camera_pose(params, curr_time_idx, forward_prop)                :1354-1373
    update_poses(params, sliding_window_kf)                                    :57-70
    matrix_to_quaternion(matrix)                                               what the use_gt_poses branch needs (:1895-1904)
    is_keyframe(time_idx, num_frames, keyframe_every, gt_w2c=None)             the rule of :2108-2109
    SlamSession(config, intrinsics, first_frame_w2c, cam)                      the body of the frame loop, :1762-2124:
        step(frame)            pose seeding, track_frame, map_frame (every map_every frames), add_keyframe, in the reference's order;
                               the first call (frame id 0) builds the map from the frame and maps it without densification
        track_frame(frame)     :1808-1904      map_frame(frame)     :1927-2083      add_keyframe(frame)     :2107-2124

`config` is a dict with the reference's key names (configs/*/*.py): tracking / mapping (num_iters, lrs, loss_weights, sil_thres,
use_sil_for_loss, use_l1, ignore_outlier_depth_loss; tracking: forward_prop, use_gt_poses, use_depth_loss_thres, depth_loss_thres;
mapping: add_new_gaussians, prune_gaussians, pruning_dict, use_gaussian_splatting_densification, densify_dict), map_every,
keyframe_every, mapping_window_size, scene_radius_depth_ratio, mean_sq_dist_method, gaussian_distribution, model.flag_use_embedding.
Three values the reference takes from its dataset object are keys here, since there is no dataset code: data.num_frames (or num_frames),
num_semantic (absent or None: a map without semantics; an int: flat classes; a list: the classes per tree level, K = their sum) and
num_semantic_class (the leaf head's classes, with model.flag_use_embedding = 1).

A frame is a dict: 'id' (its time index), 'im' [3,H,W] in 0..1, 'depth' [1,H,W], both float32 on the device; optional 'gt_w2c' [4,4]
(relative to frame 0; read by use_gt_poses and by the keyframe rule's validity test) and 'semantic_label_gt' [levels (+1 leaf),H,W].

No dataset code, no logging service, no plotting, no checkpoint resume.  There is no CPU path for anything that renders; the pose seeding,
the keyframe rule and the config handling are plain torch / Python and run anywhere.
"""
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
    cfg.setdefault('num_semantic', None)
    if cfg['num_semantic'] is not None and cfg['model']['flag_use_embedding'] == 1 and 'num_semantic_class' not in cfg:
        raise KeyError("config['num_semantic_class']")
    if int(cfg['mapping_window_size']) < 2:
        raise ValueError("mapping_window_size counts the last keyframe and the current frame: at least 2")
    return cfg


def _param_groups(params, lrs):
    """initialize_optimizer's groups (scripts/hierslam.py:411-417): one named group per parameter"""
    return [{'params': [v], 'name': k, 'lr': lrs[k]} for k, v in params.items()]


# ---- the session ----------------------------------------------------------------------------------------------------------------------
class SlamSession:
    """The state of one run and the per-frame steps (module docstring).  After each call: `params`, `variables`, `keyframe_list`,
    `keyframe_time_indices`, `gt_w2c_all_frames`, `optimizer` (the last one built), `last_window` = (selected_time_idx,
    selected_keyframes) of the last mapping step, `num_tracking_iters` of the last tracked frame."""

    def __init__(self, config, intrinsics, first_frame_w2c, cam):
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

    # -- first frame --
    def initialize(self, frame):
        cfg = self.config
        self.params, self.variables = initialize_first_timestep(
            frame['im'], frame['depth'], self.intrinsics, self.first_frame_w2c, self.num_frames, cfg['scene_radius_depth_ratio'],
            cfg['mean_sq_dist_method'], cfg['gaussian_distribution'], self.num_semantic)
        if self.flag_use_semantic and cfg['model']['flag_use_embedding'] == 1:      # :1755-1758
            dev = self.params['means3D'].device
            self.mlp = torch.nn.Conv2d(self.num_semantic, int(cfg['num_semantic_class']), kernel_size=1).to(dev)
            self.mlp_optimizer = torch.optim.Adam(self.mlp.parameters(), lr=5e-4)
        return self.params, self.variables

    # -- rendering and losses --
    def _render(self, time_idx, gaussians_grad, camera_grad, retain_means2D=False):
        from diff_gaussian_rasterization import GaussianRasterizer, GaussianRasterizer_semantic
        from . import slam_helpers as SH
        tg = SH.transform_to_frame(self.params, time_idx, gaussians_grad=gaussians_grad, camera_grad=camera_grad)
        if self.flag_use_semantic:
            rv = SH.transformed_params2rendervar_semantic(self.params, tg)
            if retain_means2D:
                rv['means2D'].retain_grad()
            im, radius, sem, depth, _median, opac = GaussianRasterizer_semantic(raster_settings=self.cam)(**rv)
        else:
            rv = SH.transformed_params2rendervar(self.params, tg)
            if retain_means2D:
                rv['means2D'].retain_grad()
            im, radius, depth, _median, opac, _mask = GaussianRasterizer(raster_settings=self.cam)(**rv)
            sem = None
        return rv, im, radius, sem, depth, opac

    def render(self, time_idx):
        """(im, depth, final opacity, semantic | None) of the map from the estimated pose of frame time_idx, without gradients"""
        with torch.no_grad():
            _rv, im, _radius, sem, depth, opac = self._render(time_idx, False, False)
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
        """the ignore_outlier_depth_loss mask (:910-913)"""
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
        mask = self._outlier_mask(frame['depth'], depth.detach())
        if trk['use_sil_for_loss']:
            mask = mask & (opac.detach() > trk['sil_thres'])
        d = L.masked_l1(depth, frame['depth'], mask, "sum")
        c = L.masked_l1(im, frame['im'], mask, "sum")
        return L.weighted_sum((d, c), (lw['depth'], lw['im'])), torch.stack((d.detach(), c.detach()))

    def _mapping_loss(self, data, im, sem, depth, it):
        from . import losses as L
        mp = self.config['mapping']
        lw = mp['loss_weights']
        if mp['ignore_outlier_depth_loss']:
            d = L.masked_l1(depth, data['depth'], self._outlier_mask(data['depth'], depth.detach()), "mean")
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
        it, extended = 0, False
        while True:
            rv, im, radius, _sem, depth, opac = self._render(time_idx, gaussians_grad=False, camera_grad=True)
            loss, parts = self._tracking_loss(frame, im, depth, opac)
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
            data = {'cam': self.cam, 'im': frame['im'], 'depth': frame['depth'], 'id': time_idx, 'intrinsics': self.intrinsics,
                    'w2c': self.first_frame_w2c}
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
        for it in range(int(mp['num_iters'])):
            pick = selected_keyframes[np.random.randint(0, len(selected_keyframes))]
            if pick == -1:
                data = frame
                iter_time_idx = time_idx
            else:
                kf = self.keyframe_list[pick]
                iter_time_idx = kf['id']
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


__all__ = ["initialize_first_timestep", "initialize_camera_pose", "update_poses", "matrix_to_quaternion", "is_keyframe", "is_mapping_frame",
           "normalize_config", "map_init_frame", "frame_w2c", "SlamSession"]
