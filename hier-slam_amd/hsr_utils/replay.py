"""A headless replay of a finished run, on the device (include/ext/hsr_replay.h): what the reference's
viz_scripts/online_recon*.py and final_recon.py do for every step of a run, without Open3D and without a window — the map as it stood
at step t (get_rendervars[_semantic], online_recon_sem_replica.py:100-158), rendered from the estimated pose or a follow camera
(render / render_semantic, :174-217), and the rendered view as a coloured world-space point cloud (rgbd2pcd, :220-259).

    run_w2cs(params)                                          [T,4,4]: the estimated poses of load_scene_data (:76-84)
    ReplayPlan(timestep, num_frames)                          ONE hsr_replay_plan, one host read: .counts[t] = the Gaussians step t shows
    replay_rendervars(params, plan, step, semantic=, w2c=None)    ONE hsr_replay_select: the rendervar dictionary of step `step`
    replay_view(params, plan, step, w2c, k, w, h, semantic=, ...) (im, depth, im_semantic | None, silhouette) of that map from w2c
    view_cloud(depth, k, w2c, picture=None, records=False)    ONE hsr_replay_cloud: the points, or the PLY records with the picture's colours
    save_cloud_ply(path, records)                             header, one device-to-host copy, one write
    follow_camera(first_view_w2c, w2c_t)                      the matrix product of :375
    camera_centres(w2cs), trajectory_lines(n)                 the trajectory of :348 and make_lineset (:161-171): host-side and tiny
    replay_run(params, out_dir, every=, semantic=, picture=, cloud=, follow=, ...)    the loop of visualize (:262-410) without the window

Output tensors are sized from the plan, so no step reads a count back.  Not copied from the reference (the header says why): the
per-view jet re-normalisation of render_mode='depth', and the unselected params['semantic'] of get_rendervars_semantic — here the
semantic rows are selected like the rest.  There is no CPU path for anything that launches; the pose and trajectory helpers are plain
torch / numpy and run anywhere.
"""
import os

import numpy as np
import torch

from diff_gaussian_rasterization import _abi

_lib = _abi.lib

REPLAY_MAX_STEPS = 1 << 20      # HSR_REPLAY_MAX_STEPS
ROT_PARAMS, ROT_TRANSFORMED = 0, 1
CLOUD_FIELDS = tuple(("float", n) for n in ("x", "y", "z")) + tuple(("uchar", n) for n in ("red", "green", "blue"))
CLOUD_RECORD_BYTES = 15
PICTURES = ("color", "depth", "semantic")


def _host(m):
    """a small matrix as a numpy array on the host, whatever it came as"""
    return m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)


def _check_w2c(w2c):
    shape = tuple(w2c.shape) if hasattr(w2c, "shape") else tuple(np.asarray(w2c).shape)
    if shape != (4, 4):
        raise RuntimeError("hsr_utils.replay: w2c must be [4,4] (got %s)" % (shape,))


def _p(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def run_w2cs(params):
    """[T,4,4] float32 where the pose parameters live: the estimated world-to-camera of every frame, slam.frame_w2c(params, t) for
    t = 0 .. T-1 (load_scene_data, :76-84).  Once per run."""
    from . import slam
    T = int(params['cam_unnorm_rots'].shape[-1])
    return torch.stack([slam.frame_w2c(params, t) for t in range(T)]).to(torch.float32)


class ReplayPlan:
    """How many Gaussians each step of a run shows: counts[t] = #{p : timestep[p] <= t} for t = 0 .. num_frames - 1, a numpy int64
    array, from one hsr_replay_plan and one host read.  `timestep` is the float32 device tensor [P] (params['timestep'] of a finished
    run, variables['timestep'] of a session); it is kept as .timestep."""

    def __init__(self, timestep, num_frames):
        T = int(num_frames)
        if not 1 <= T <= REPLAY_MAX_STEPS:
            raise ValueError("hsr_utils.replay: num_frames must be 1..%d (got %d)" % (REPLAY_MAX_STEPS, T))
        if not isinstance(timestep, torch.Tensor) or timestep.dim() != 1:
            raise RuntimeError("hsr_utils.replay: timestep must be a tensor [P]")
        if not timestep.is_cuda or timestep.dtype != torch.float32:
            raise RuntimeError("hsr_utils.replay: timestep must be float32 on a HIP device (got %s on %s); there is no CPU path"
                               % (timestep.dtype, timestep.device))
        self.timestep = timestep.detach().contiguous()
        dev, P = self.timestep.device, int(self.timestep.numel())
        upto = torch.empty(T, dtype=torch.int64, device=dev)
        scratch = torch.empty(int(_lib.hsr_replay_plan_scratch_bytes(P, T)), dtype=torch.uint8, device=dev)
        _abi.call(_lib.hsr_replay_plan, "hsr_replay_plan", dev, P, T, _p(self.timestep), upto.data_ptr(), scratch.data_ptr(), scratch.numel())
        self.counts = upto.cpu().numpy()      # the one host read of the run
        self.num_frames = T

    def __len__(self):
        return self.num_frames


def _map_arrays(params, plan, step, semantic):
    """the host-side argument checks of a step, before anything touches the device; returns (P, S, K, step)"""
    if not isinstance(plan, ReplayPlan):
        raise RuntimeError("hsr_utils.replay: plan must be a ReplayPlan")
    P = int(params['means3D'].shape[0])
    if int(plan.timestep.numel()) != P:
        raise RuntimeError("hsr_utils.replay: timestep has %d entries, the map %d Gaussians" % (plan.timestep.numel(), P))
    step = int(step)
    if not 0 <= step < len(plan):
        raise ValueError("hsr_utils.replay: step %d is outside the plan's 0..%d" % (step, len(plan) - 1))
    if semantic and 'semantic' not in params:
        raise RuntimeError("hsr_utils.replay: semantic=True needs params['semantic']")
    ls = params['log_scales']
    if ls.dim() != 2 or ls.shape[0] != P or ls.shape[1] not in (1, 3):
        raise RuntimeError("hsr_utils.replay: log_scales must be [P,1] or [P,3] (got %s)" % (tuple(ls.shape),))
    K = int(params['semantic'].shape[1]) if semantic else 0
    return P, int(ls.shape[1]), K, step


def replay_rendervars(params, plan, step, *, semantic, w2c=None):
    """The rendervar dictionary of get_rendervars / get_rendervars_semantic (:100-158) for the map as it stood at `step`: the keys of
    slam_helpers.transformed_params2rendervar[_semantic] ('means2D' zeros), every tensor holding the plan.counts[step] rows with
    timestep <= step in their original order, from ONE hsr_replay_select.  w2c=None leaves the map in the world frame, as the viewer
    does (the pose goes to the camera); a w2c ([4,4], slam_helpers.transform_to_view's rules) puts it in that camera's frame, as the SLAM
    loop does.  The rotations are those of transformed_params2rendervar (semantic: F.normalize of the stored ones).  No host read."""
    from .slam_helpers import _dev_f32, _view_matrix
    if w2c is not None:
        _check_w2c(w2c)
    P, S, K, step = _map_arrays(params, plan, step, semantic)
    with torch.no_grad():
        means3D = _dev_f32(params['means3D'].detach(), "means3D")
        dev = means3D.device
        rots = _dev_f32(params['unnorm_rotations'].detach(), "unnorm_rotations")
        logit = _dev_f32(params['logit_opacities'].detach(), "logit_opacities")
        ls = _dev_f32(params['log_scales'].detach(), "log_scales")
        rgb = _dev_f32(params['rgb_colors'].detach(), "rgb_colors")
        sem = _dev_f32(params['semantic'].detach(), "semantic") if semantic else None
        if plan.timestep.device != dev:
            raise RuntimeError("hsr_utils.replay: the plan is on %s, the map on %s" % (plan.timestep.device, dev))
        view = None if w2c is None else _view_matrix(w2c, dev)
        n = int(plan.counts[step])
        o = dict(dtype=torch.float32, device=dev)
        out = {'means3D': torch.empty((n, 3), **o), 'colors_precomp': torch.empty((n, 3), **o), 'rotations': torch.empty((n, 4), **o),
               'opacities': torch.empty((n, 1), **o), 'scales': torch.empty((n, 3), **o)}
        if semantic:
            out['semantics_precomp'] = torch.empty((n, K), **o)
        out['means2D'] = torch.zeros((n, 3), **o)
        count = torch.empty(1, dtype=torch.int32, device=dev)      # required by the ABI; sized from the plan, it is not read
        scratch = torch.empty(int(_lib.hsr_replay_select_scratch_bytes(P)), dtype=torch.uint8, device=dev)
        _abi.call(_lib.hsr_replay_select, "hsr_replay_select", dev, P, S, K, int(S != 1 and view is not None),
                  ROT_PARAMS if semantic else ROT_TRANSFORMED, step, n, _p(plan.timestep), _p(means3D), _p(rots), _p(logit), _p(ls), _p(rgb),
                  _p(sem), None if view is None else view.data_ptr(), _p(out['means3D']), None, _p(out['rotations']), _p(out['opacities']),
                  _p(out['scales']), _p(out['colors_precomp']), _p(out.get('semantics_precomp')), None, count.data_ptr(),
                  scratch.data_ptr(), scratch.numel())
    return out


def replay_view(params, plan, step, w2c, k, w, h, *, semantic, near=0.01, far=100, white_bg=True):
    """(im, depth, im_semantic | None, silhouette) of the map as it stood at `step`, seen from w2c with the pinhole k ([3,3]) at w x h:
    render / render_semantic (:174-217) on the world-frame rendervar and camera.setup_camera(w, h, k, w2c, near, far), the background
    white as there.  The silhouette is the rasterizer's final opacity.  Under torch.no_grad()."""
    from diff_gaussian_rasterization import GaussianRasterizer, GaussianRasterizer_semantic
    from .camera import setup_camera
    _check_w2c(w2c)
    _map_arrays(params, plan, step, semantic)
    with torch.no_grad():
        rv = replay_rendervars(params, plan, step, semantic=semantic)
        dev = rv['means3D'].device
        cam = setup_camera(w, h, _host(k), _host(w2c), near, far, device=dev)
        if white_bg:
            cam = cam._replace(bg=torch.ones(3, dtype=torch.float32, device=dev))
        if semantic:
            im, _radius, sem, depth, _median, opac = GaussianRasterizer_semantic(raster_settings=cam)(**rv)
        else:
            im, _radius, depth, _median, opac, _mask = GaussianRasterizer(raster_settings=cam)(**rv)
            sem = None
    return im, depth, sem, opac


def view_cloud(depth, k, w2c, picture=None, records=False):
    """rgbd2pcd (:220-259) in ONE launch: every pixel (x, y) of depth ([1,H,W] or [H,W], float32 on the device) back-projected with the
    pinhole k and c2w = torch.linalg.inv(w2c) (on the device, as in the reference).  Returns the points, float32 [H*W,3]; with
    records=True the body of a PLY file instead, uint8 [H*W,15]: x, y, z and the pixel's red, green, blue from `picture` (uint8 [H,W,3],
    an export_frame picture).  A zero depth lands on the camera centre, as in the reference."""
    if records and picture is None:
        raise RuntimeError("hsr_utils.replay: records=True needs a picture (uint8 [H,W,3])")
    _check_w2c(w2c)
    from .evaluate import _dev, _plane
    from .slam_helpers import _view_matrix
    if not isinstance(depth, torch.Tensor) or depth.dim() < 2:
        raise RuntimeError("hsr_utils.replay: depth must be a tensor [1,H,W] or [H,W]")
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    depth = _plane(depth.detach(), "depth", H, W)
    dev = depth.device
    if records:
        picture = _dev(picture, "picture", torch.uint8)
        if tuple(picture.shape) != (H, W, 3) or picture.device != dev:
            raise RuntimeError("hsr_utils.replay: picture must be uint8 [%d,%d,3] on %s (got %s on %s)" % (H, W, dev, tuple(picture.shape), picture.device))
    kh = _host(k)
    c2w = torch.linalg.inv_ex(_view_matrix(w2c, dev)).inverse.contiguous()      # torch.linalg.inv without its host read of the status
    out = torch.empty((H * W, CLOUD_RECORD_BYTES), dtype=torch.uint8, device=dev) if records else torch.empty((H * W, 3), dtype=torch.float32, device=dev)
    _abi.call(_lib.hsr_replay_cloud, "hsr_replay_cloud", dev, H, W, depth.data_ptr(), picture.data_ptr() if records else None, float(kh[0][0]),
              float(kh[1][1]), float(kh[0][2]), float(kh[1][2]), c2w.data_ptr(), None if records else out.data_ptr(),
              out.data_ptr() if records else None)
    return out


def save_cloud_ply(path, records):
    """view_cloud(..., records=True)'s bytes as a PLY file: map_export.ply_header, one device-to-host copy of the body, one write"""
    from .map_export import ply_header
    host = records.detach().cpu().contiguous().numpy().reshape(-1)
    if host.dtype != np.uint8 or host.size % CLOUD_RECORD_BYTES:
        raise RuntimeError("hsr_utils.replay: records must be uint8 [n,15] (got %s of %d bytes)" % (host.dtype, host.size))
    with open(path, "wb") as f:
        f.write(ply_header(host.size // CLOUD_RECORD_BYTES, CLOUD_FIELDS))
        f.write(memoryview(host))
    return path


def follow_camera(first_view_w2c, w2c_t):
    """the viewer's camera at step t (:375): np.dot(first_view_w2c, all_w2cs[t]); tensors give a tensor, arrays an array"""
    _check_w2c(first_view_w2c)
    _check_w2c(w2c_t)
    if isinstance(first_view_w2c, torch.Tensor) or isinstance(w2c_t, torch.Tensor):
        a = torch.as_tensor(first_view_w2c)
        b = torch.as_tensor(w2c_t)
        return a.to(b.device) @ b if isinstance(w2c_t, torch.Tensor) else a @ b.to(a.device)
    return np.dot(first_view_w2c, w2c_t)


def camera_centres(w2cs):
    """[T,3]: np.linalg.inv(w2c)[:3, 3] of every pose (:348), on the host"""
    w2cs = _host(w2cs)
    if w2cs.ndim != 3 or w2cs.shape[1:] != (4, 4):
        raise RuntimeError("hsr_utils.replay: w2cs must be [T,4,4] (got %s)" % (w2cs.shape,))
    return np.stack([np.linalg.inv(m)[:3, 3] for m in w2cs]) if len(w2cs) else np.zeros((0, 3), w2cs.dtype)


def trajectory_lines(n):
    """int32 [n-1,2]: the index pairs of make_lineset (:161-171) with one line per step, (t, t - 1) for t = 1 .. n-1"""
    pt_indices = np.arange(int(n))
    return np.ascontiguousarray(np.stack((pt_indices, pt_indices - 1), -1)[1:], np.int32)


def replay_run(params, out_dir, *, every=1, semantic=False, picture="color", cloud=False, follow=None, steps=None, timestep=None,
               intrinsics=None, width=None, height=None, num_frames=None, near=0.01, far=100, **export_kw):
    """The loop of visualize (:262-410) without the window.  For every `every`-th step t of the run (or the given `steps`) the map as it
    stood at t is rendered from the estimated pose of frame t — with follow=first_view_w2c from follow_camera(follow, pose), the
    viewer's camera — and out_dir/{t}.png is written through export_frame and write_png; with cloud=True also out_dir/{t}.ply, the
    rendered depth back-projected and coloured by that picture.  picture: "color", "depth" (export_kw: depth_range, depth_table) or
    "semantic" (needs semantic=True and export_kw level_sizes and tuple_table).  params is the dictionary of a finished run
    (map_io.load_params(path, device)); timestep, intrinsics, width, height and num_frames default to its 'timestep', 'intrinsics',
    'org_width', 'org_height' and the number of pose columns.  A step that shows no Gaussian yet is skipped.  Returns the list of
    steps written; final_recon.py is steps=[T - 1]."""
    from . import export
    if picture not in PICTURES:
        raise ValueError("hsr_utils.replay: picture must be one of %s (got %r)" % (", ".join(PICTURES), picture))
    if picture == "semantic" and not semantic:
        raise ValueError("hsr_utils.replay: picture='semantic' needs semantic=True")
    if int(every) < 1:
        raise ValueError("hsr_utils.replay: every must be >= 1")
    if timestep is None:
        if 'timestep' not in params:
            raise RuntimeError("hsr_utils.replay: the run carries no 'timestep' (pass timestep=)")
        timestep = params['timestep']
    P = int(params['means3D'].shape[0])
    if int(timestep.numel()) != P:
        raise RuntimeError("hsr_utils.replay: timestep has %d entries, the map %d Gaussians" % (timestep.numel(), P))
    if semantic and 'semantic' not in params:
        raise RuntimeError("hsr_utils.replay: semantic=True needs params['semantic']")
    if follow is not None:
        _check_w2c(follow)
    k = _host(params['intrinsics'] if intrinsics is None else intrinsics)[:3, :3]
    w = int(_host(params['org_width'])) if width is None else int(width)
    h = int(_host(params['org_height'])) if height is None else int(height)
    T = int(params['cam_unnorm_rots'].shape[-1]) if num_frames is None else int(num_frames)
    steps = list(range(0, T, int(every))) if steps is None else [int(t) for t in steps]
    for t in steps:
        if not 0 <= t < T:
            raise ValueError("hsr_utils.replay: step %d is outside the run's 0..%d" % (t, T - 1))
    os.makedirs(out_dir, exist_ok=True)
    poses = run_w2cs(params).cpu().numpy()      # one copy for the run
    plan = ReplayPlan(timestep.detach().reshape(-1), T)
    follow = None if follow is None else _host(follow).astype(np.float32)
    written = []
    for t in steps:
        if plan.counts[t] == 0:
            continue
        view = poses[t] if follow is None else follow_camera(follow, poses[t])
        im, depth, sem, _sil = replay_view(params, plan, t, view, k, w, h, semantic=semantic, near=near, far=far)
        if picture == "color":
            pic = export.export_frame(im=im)["im"]
        elif picture == "depth":
            pic = export.export_frame(depth=depth, **export_kw)["depth"]
        else:
            pic = export.export_frame(im_semantic=sem, **export_kw)["im_semantic"]
        export.write_png(os.path.join(out_dir, "%d.png" % t), pic)
        if cloud:
            save_cloud_ply(os.path.join(out_dir, "%d.ply" % t), view_cloud(depth, k, view, picture=pic, records=True))
        written.append(t)
    return written


__all__ = ["run_w2cs", "ReplayPlan", "replay_rendervars", "replay_view", "view_cloud", "save_cloud_ply", "follow_camera", "camera_centres",
           "trajectory_lines", "replay_run", "CLOUD_FIELDS"]
