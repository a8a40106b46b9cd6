"""Checkpoint and resume of a SLAM session, and the packed keyframe store they stand on (include/ext/hsr_keyframe_pack.h, DESIGN.md §7
row 13).  The reference saves params{t}.npz and keyframe_time_indices{t}.npy every checkpoint_interval frames (scripts/hierslam.py:2128-2133)
and, to resume, re-reads every earlier frame from its dataset (:1716-1752); it drops the keyframes' label planes, zeroes
variables['timestep'] and forgets the leaf head's Adam state and the random streams.  Here a third file, session{t}.npz, holds what those
two lack, so that a resumed session continues as the saved one would have.

    pack_keyframe(color, depth, labels=None, depth_scale=None)     ONE hsr_keyframe_pack call -> PackedKeyframe
    unpack_keyframe(pk)                                            ONE hsr_keyframe_unpack launch -> (color, depth, labels | None), bit-equal
    PackedKeyframe                                                 .exact {'color', 'depth', 'labels'}: which groups are held as codes
    save_checkpoint(session, directory, time_idx=None)             params{t}.npz, keyframe_time_indices{t}.npy, session{t}.npz
    load_checkpoint(session, directory, time_idx, frames=None)     into a freshly constructed session; without session{t}.npz the
                                                                   reference's own resume, from frames(i)

A keyframe of H x W pixels with L label planes is 12 + 4 + 8 L bytes per pixel as float32 / int64 planes and 3 + 2 + 2 L as codes.  The
codes are exact for a frame that came through ingest() at sensor size (its colour is float(v) / 255 for an 8-bit v, its depth
float(double(q) / png_depth_scale) for a 16-bit q); the pack call counts, per group, the values its codes do not reproduce, and a
group with a non-zero count is kept as it came (a bilinearly resized ScanNet colour image, a rendered depth): the packed form is ALWAYS
exact.  The counts stay on the device until something needs them (PackedKeyframe.resolve: one host read, long after the launch).

session{t}.npz holds arrays only (np.load(..., allow_pickle=False) reads it).  Its entries:
    time_idx, fingerprint.{num_frames, height, width, num_semantic, scale_columns, frames}
    var.<name>                    every tensor of session.variables but the per-iteration 'means2D' and 'seen'; scene_radius
    gt_w2c [F,4,4], gt_w2c_mask   the ground-truth poses seen so far; the mask is False where a frame had none
    keyframe_time_indices, kf.ids, kf.est_w2c [n,4,4], kf.depth_scale [n] (NaN: none)
    kf<i>.color_u8 | kf<i>.color_raw, kf<i>.depth_u16 | kf<i>.depth_raw, kf<i>.labels_u16 | kf<i>.labels_raw (absent: no labels)
    mlp.weight, mlp.bias, mlp.<exp_avg | exp_avg_sq | step>.<weight | bias>      the leaf head and its Adam state, when there is one
    rng.np_keys, rng.np_pos, rng.np_gauss, rng.torch (, rng.torch_device)         np.random.get_state(), torch.get_rng_state() and the
                                                                                  device generator's state
There is no CPU path for the two kernels; saving and loading are host work and run anywhere (host keyframes are stored as they are).
"""
import os

import numpy as np
import torch

from diff_gaussian_rasterization import _abi

_lib = _abi.lib

MAX_SIDE = 16384        # HSR_KEYFRAME_MAX_SIDE
MAX_PLANES = 17         # HSR_KEYFRAME_MAX_PLANES
GROUPS = ("color", "depth", "labels")
SKIPPED_VARIABLES = ("means2D", "seen", "scene_radius")      # per-iteration tensors; scene_radius has an entry of its own
BOOKKEEPING = ("max_2D_radius", "means2D_gradient_accum", "denom", "timestep")
PACK_BATCH = 16         # keyframes of a raw store packed per round of save_checkpoint: 16 x 12 MB of codes on the device at 1200x680


# ---- the packed keyframe ---------------------------------------------------------------------------------------------------------------
class PackedKeyframe:
    """One keyframe's planes, each group (colour [3,H,W] float32, depth [1,H,W] float32, labels [L,H,W] int64 or None) held either as
    codes (.codes[group]: uint8 / uint16 / uint16, stored as int16 bit patterns) or as it came (.raw[group]).  Until resolve() both may
    be there: the counts that decide are still on the device (.lossy, int32 [3] holding uint32 bit patterns)."""

    def __init__(self, H, W, depth_scale, codes, raw, lossy, depth_shape):
        self.H, self.W, self.depth_scale = int(H), int(W), depth_scale
        self.codes, self.raw, self.lossy, self.depth_shape = codes, raw, lossy, tuple(depth_shape)
        self._exact = None if lossy is not None else {g: g in codes for g in GROUPS if g in codes or g in raw}

    def resolve(self):
        """decide each group from its count (the one host read) and drop the half not needed; returns self"""
        if self._exact is None:
            counts = self.lossy.cpu().numpy().view(np.uint32)
            self._exact = {}
            for k, g in enumerate(GROUPS):
                if g in self.codes and int(counts[k]) == 0:
                    self._exact[g] = True
                    self.raw.pop(g, None)
                elif g in self.raw:
                    self._exact[g] = False
                    self.codes.pop(g, None)
        return self

    @property
    def exact(self):
        """{'color': bool, 'depth': bool (, 'labels': bool)}: True where the group is held as codes"""
        return dict(self.resolve()._exact)

    @property
    def lossy_counts(self):
        """(colour values, depth pixels, label values) the codes did not reproduce, as Python ints; None for a keyframe never packed"""
        return None if self.lossy is None else tuple(int(c) for c in self.lossy.cpu().numpy().view(np.uint32))

    def nbytes(self):
        self.resolve()
        return sum(t.numel() * t.element_size() for part in (self.codes, self.raw) for t in part.values())


def _plane_checks(color, depth, labels):
    if not (torch.is_tensor(color) and torch.is_tensor(depth)):
        raise RuntimeError("hsr_utils.checkpoint: color and depth must be tensors")
    H, W = depth.shape[-2:]
    if tuple(color.shape) != (3, H, W) or depth.numel() != H * W:
        raise RuntimeError("hsr_utils.checkpoint: color must be [3,H,W] and depth [H,W] or [1,H,W]; got %s and %s"
                           % (tuple(color.shape), tuple(depth.shape)))
    if labels is not None and (not torch.is_tensor(labels) or labels.dim() != 3 or tuple(labels.shape[1:]) != (H, W)):
        raise RuntimeError("hsr_utils.checkpoint: labels must be [L,%d,%d]; got %s" % (H, W, tuple(getattr(labels, 'shape', ()))))
    return int(H), int(W)


def raw_keyframe(color, depth, labels=None):
    """a PackedKeyframe that holds its planes as they came: what a host tensor, or a keyframe loaded from raw entries, becomes"""
    H, W = _plane_checks(color, depth, labels)
    raw = {"color": color, "depth": depth}
    if labels is not None:
        raw["labels"] = labels
    return PackedKeyframe(H, W, None, {}, raw, None, depth.shape)


def pack_keyframe(color, depth, labels=None, depth_scale=None):
    """A PackedKeyframe of colour [3,H,W] float32, depth [H,W] or [1,H,W] float32 and labels int64 [L,H,W] (or None), from ONE
    hsr_keyframe_pack call and no host read.  depth_scale is the png_depth_scale the depth was ingested with; None keeps the depth as
    it is.  Labels that are not int64, or more than 17 planes, stay as they are.  The inputs are referenced, not copied, until
    resolve() has seen the counts."""
    H, W = _plane_checks(color, depth, labels)
    if not (color.is_cuda and depth.is_cuda and color.dtype == torch.float32 and depth.dtype == torch.float32) \
            or (labels is not None and not labels.is_cuda):
        raise RuntimeError("hsr_utils.checkpoint: color and depth must be float32 tensors on a HIP device (labels on it too); "
                           "there is no CPU path")
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError("hsr_utils.checkpoint: sides must be 1..%d; got %dx%d" % (MAX_SIDE, H, W))
    if depth_scale is not None:
        depth_scale = float(depth_scale)
        if not np.isfinite(depth_scale) or depth_scale == 0.0:
            raise ValueError("hsr_utils.checkpoint: depth_scale must be finite and non-zero; got %r" % depth_scale)
    dev = color.device
    raw = {"color": color, "depth": depth}
    col, d = color.detach().contiguous(), (depth.detach().reshape(H, W).contiguous() if depth_scale is not None else None)
    lab = None
    if labels is not None:
        raw["labels"] = labels
        if labels.dtype == torch.int64 and 1 <= labels.shape[0] <= MAX_PLANES:
            lab = labels.detach().contiguous()
    L = 0 if lab is None else int(lab.shape[0])
    codes = {"color": torch.empty((3, H, W), dtype=torch.uint8, device=dev)}
    if d is not None:
        codes["depth"] = torch.empty((H, W), dtype=torch.int16, device=dev)
    if lab is not None:
        codes["labels"] = torch.empty((L, H, W), dtype=torch.int16, device=dev)
    lossy = torch.empty(3, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(_lib.hsr_keyframe_pack_scratch_bytes(H, W, L)), dtype=torch.uint8, device=dev)
    _abi.call(_lib.hsr_keyframe_pack, "hsr_keyframe_pack", dev, H, W, col.data_ptr(), None if d is None else d.data_ptr(), L,
              None if lab is None else lab.data_ptr(), 1.0 if depth_scale is None else depth_scale, codes["color"].data_ptr(),
              None if d is None else codes["depth"].data_ptr(), None if lab is None else codes["labels"].data_ptr(), lossy.data_ptr(),
              scratch.data_ptr(), scratch.numel())
    return PackedKeyframe(H, W, depth_scale, codes, raw, lossy, depth.shape)


def unpack_keyframe(pk):
    """(color [3,H,W] float32, depth in its original shape, labels int64 [L,H,W] | None) of a PackedKeyframe, bit-equal to what was
    packed: the groups held as codes from ONE hsr_keyframe_unpack launch (none when no group is), the others as they were kept."""
    pk.resolve()
    H, W = pk.H, pk.W
    c, d, lab = pk.codes.get("color"), pk.codes.get("depth"), pk.codes.get("labels")
    out = dict(pk.raw)
    if c is not None or d is not None or lab is not None:
        dev = (c if c is not None else d if d is not None else lab).device
        if dev.type != "cuda":
            raise RuntimeError("hsr_utils.checkpoint: the codes must be on a HIP device; there is no CPU path")
        if c is not None:
            out["color"] = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        if d is not None:
            out["depth"] = torch.empty(pk.depth_shape, dtype=torch.float32, device=dev)
        L = 0 if lab is None else int(lab.shape[0])
        if lab is not None:
            out["labels"] = torch.empty((L, H, W), dtype=torch.int64, device=dev)
        _abi.call(_lib.hsr_keyframe_unpack, "hsr_keyframe_unpack", dev, H, W, None if c is None else c.data_ptr(),
                  None if d is None else d.data_ptr(), L, None if lab is None else lab.data_ptr(),
                  1.0 if pk.depth_scale is None else pk.depth_scale, None if c is None else out["color"].data_ptr(),
                  None if d is None else out["depth"].data_ptr(), None if lab is None else out["labels"].data_ptr())
    return out["color"], out["depth"], out.get("labels")


# ---- the session's keyframes in either store -------------------------------------------------------------------------------------------
def keyframe_planes(kf):
    """(color, depth, labels | None) of a keyframe_list entry of either store"""
    if 'packed' in kf:
        return unpack_keyframe(kf['packed'])
    return kf['color'], kf['depth'], kf.get('label_gt')


def _packed_of(kf, depth_scale):
    """the PackedKeyframe of a keyframe_list entry: its own under the packed store, else packed now (device) or kept raw (host)"""
    if 'packed' in kf:
        return kf['packed']
    color, depth, labels = kf['color'], kf['depth'], kf.get('label_gt')
    if torch.is_tensor(color) and color.is_cuda:
        return pack_keyframe(color, depth, labels, depth_scale)
    return raw_keyframe(color, depth, labels)


def _np(t):
    return t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.asarray(t)


def _session_device(session):
    view = getattr(session.cam, 'viewmatrix', None)
    return view.device if torch.is_tensor(view) else torch.device("cpu")


def _fingerprint(session, frames):
    from . import slam
    cfg = session.config
    return {"num_frames": session.num_frames, "height": int(session.cam.image_height), "width": int(session.cam.image_width),
            "num_semantic": -1 if session.num_semantic is None else int(session.num_semantic),
            "scale_columns": slam._scale_columns(cfg['gaussian_distribution'], session.flag_use_semantic), "frames": int(frames)}


def save_checkpoint(session, directory, time_idx=None):
    """Write params{t}.npz (map_io.save_params_ckpt: the reference loads it), keyframe_time_indices{t}.npy (:2131) and session{t}.npz
    (module docstring) into `directory`; t defaults to the last frame stepped, and no other value is accepted once frames were stepped:
    the files describe the session as it stands.  Draws from no random stream and changes nothing in the session.  Returns the three paths."""
    from . import map_io
    if session.params is None:
        raise RuntimeError("hsr_utils.checkpoint: save_checkpoint before the first frame: there is no map yet")
    frames = len(session.gt_w2c_all_frames)
    t = frames - 1 if time_idx is None else int(time_idx)
    if t != frames - 1:
        raise ValueError("hsr_utils.checkpoint: the session stands after frame %d; it cannot be saved as frame %d" % (frames - 1, t))
    os.makedirs(directory, exist_ok=True)
    p_path = map_io.save_params_ckpt(session.params, directory, t)
    k_path = os.path.join(directory, "keyframe_time_indices%d.npy" % t)
    np.save(k_path, np.array(session.keyframe_time_indices))

    out = {"time_idx": np.int64(t)}
    for k, v in _fingerprint(session, frames).items():
        out["fingerprint." + k] = np.int64(v)
    for k, v in session.variables.items():
        if k not in SKIPPED_VARIABLES and torch.is_tensor(v):
            out["var." + k] = _np(v)
    out["scene_radius"] = _np(session.variables['scene_radius'])
    mask = np.array([g is not None for g in session.gt_w2c_all_frames], dtype=bool)
    gt = np.zeros((frames, 4, 4), dtype=np.float32)
    for i, g in enumerate(session.gt_w2c_all_frames):
        if g is not None:
            gt[i] = _np(g).astype(np.float32, copy=False)
    out["gt_w2c"], out["gt_w2c_mask"] = gt, mask
    out["keyframe_time_indices"] = np.array(session.keyframe_time_indices, dtype=np.int64)
    kfs = session.keyframe_list
    out["kf.ids"] = np.array([kf['id'] for kf in kfs], dtype=np.int64)
    out["kf.est_w2c"] = np.stack([_np(kf['est_w2c']) for kf in kfs]).astype(np.float32, copy=False) if kfs else np.zeros((0, 4, 4), np.float32)
    scale = session._png_depth_scale()
    scales = []
    for first in range(0, len(kfs), PACK_BATCH):      # a batch's launches first, then its reads; its codes leave the device with it
        batch = [_packed_of(kf, scale) for kf in kfs[first:first + PACK_BATCH]]
        for i, pk in enumerate(batch, start=first):
            pk.resolve()
            scales.append(np.nan if pk.depth_scale is None else pk.depth_scale)
            for g, suffix in (("color", "u8"), ("depth", "u16"), ("labels", "u16")):
                if g in pk.codes:
                    a = _np(pk.codes[g])
                    out["kf%d.%s_%s" % (i, g, suffix)] = a if suffix == "u8" else a.view(np.uint16)
                elif g in pk.raw:
                    out["kf%d.%s_raw" % (i, g)] = _np(pk.raw[g])
    out["kf.depth_scale"] = np.array(scales, dtype=np.float64)
    if session.mlp is not None:
        named = dict(session.mlp.named_parameters())
        for n, p in named.items():
            out["mlp." + n] = _np(p)
            st = session.mlp_optimizer.state.get(p, {}) if session.mlp_optimizer is not None else {}
            for m in ("exp_avg", "exp_avg_sq", "step"):
                if m in st:
                    out["mlp.%s.%s" % (m, n)] = _np(st[m])
    kind, keys, pos, has_gauss, gauss = np.random.get_state()
    if kind != "MT19937":
        raise RuntimeError("hsr_utils.checkpoint: np.random's generator is %s, not MT19937" % kind)
    out["rng.np_keys"], out["rng.np_pos"], out["rng.np_gauss"] = np.asarray(keys, np.uint32), np.array([pos, has_gauss], np.int64), np.float64(gauss)
    out["rng.torch"] = torch.get_rng_state().numpy()
    dev = session.params['means3D'].device
    if dev.type == "cuda":
        out["rng.torch_device"] = torch.cuda.get_rng_state(dev).numpy()
    s_path = os.path.join(directory, "session%d.npz" % t)
    np.savez(s_path, **out)
    return p_path, k_path, s_path


def _tensor(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)      # np.array keeps a 0-d array 0-d


def _load_params(path, dev):
    """:1721-1722: every entry of params{t}.npz as a float32 tensor on the device that requires gradients (an nn.Parameter, as the
    session's own are)"""
    z = np.load(path, allow_pickle=False)
    return {k: torch.nn.Parameter(torch.tensor(z[k]).to(dev).float().contiguous().requires_grad_(True)) for k in z.files}


def _store(session, kf, pk, labelled):
    """the keyframe_list entry of `pk` under the session's store"""
    if session.keyframe_store == "packed":
        kf['packed'] = pk
    else:
        kf['color'], kf['depth'], labels = unpack_keyframe(pk)
        if labelled:
            kf['label_gt'] = labels
    kf['cam'], kf['intrinsics'] = session.cam, session.intrinsics
    return kf


def load_checkpoint(session, directory, time_idx, frames=None):
    """Resume a freshly constructed session from the files of save_checkpoint(directory, time_idx).  With session{t}.npz everything it
    holds is restored (keyframes unpacked, or kept packed under keyframe_store="packed"; both random streams) and the next step()
    takes frame t + 1.  Without it the checkpoint is the reference's own: `frames(i)` must supply the frame dict of frame i, and
    scripts/hierslam.py:1717-1750 is done on them — the next step() takes frame t again, as the reference's loop does."""
    t = int(time_idx)
    if session.params is not None or session.gt_w2c_all_frames:
        raise RuntimeError("hsr_utils.checkpoint: load_checkpoint needs a freshly constructed session; this one has stepped %d frames"
                           % len(session.gt_w2c_all_frames))
    p_path = os.path.join(directory, "params%d.npz" % t)
    s_path = os.path.join(directory, "session%d.npz" % t)
    if not os.path.exists(p_path):
        raise FileNotFoundError(p_path)
    dev = _session_device(session)
    if not os.path.exists(s_path):
        return _load_reference_checkpoint(session, directory, t, frames, dev)
    z = np.load(s_path, allow_pickle=False)
    want = _fingerprint(session, t + 1)
    for k, v in want.items():
        got = int(z["fingerprint." + k])
        if got != v:
            raise RuntimeError("hsr_utils.checkpoint: %s was saved with %s = %d, this session has %d" % (s_path, k, got, v))
    if int(z["time_idx"]) != t:
        raise RuntimeError("hsr_utils.checkpoint: %s was saved with time_idx = %d, not %d" % (s_path, int(z["time_idx"]), t))
    session.params = _load_params(p_path, dev)
    session.variables = {k[4:]: _tensor(z[k], dev) for k in z.files if k.startswith("var.")}
    session.variables['scene_radius'] = _tensor(z["scene_radius"], dev)
    session.gt_w2c_all_frames = [(_tensor(g, dev) if m else None) for g, m in zip(z["gt_w2c"], z["gt_w2c_mask"])]
    session.keyframe_time_indices = [int(i) for i in z["keyframe_time_indices"]]
    session.keyframe_list = []
    scales = z["kf.depth_scale"]
    for i, kid in enumerate(z["kf.ids"]):
        codes, raw = {}, {}
        for g, suffix in (("color", "u8"), ("depth", "u16"), ("labels", "u16")):
            ck, rk = "kf%d.%s_%s" % (i, g, suffix), "kf%d.%s_raw" % (i, g)
            if ck in z.files:
                a = z[ck]
                codes[g] = _tensor(a if suffix == "u8" else a.view(np.int16), dev)
            elif rk in z.files:
                raw[g] = _tensor(z[rk], dev)
        H, W = (codes.get("color") if "color" in codes else raw["color"]).shape[-2:]
        pk = PackedKeyframe(H, W, None if np.isnan(scales[i]) else float(scales[i]), codes, raw, None,
                            raw["depth"].shape if "depth" in raw else (1, H, W))
        kf = {'id': int(kid), 'est_w2c': _tensor(z["kf.est_w2c"][i], dev)}
        session.keyframe_list.append(_store(session, kf, pk, session.flag_use_semantic))
    if "mlp.weight" in z.files:
        cfg = session.config
        session.mlp = torch.nn.Conv2d(session.num_semantic, int(cfg['num_semantic_class']), kernel_size=1).to(dev)
        session.mlp_optimizer = torch.optim.Adam(session.mlp.parameters(), lr=5e-4)
        with torch.no_grad():
            for n, p in session.mlp.named_parameters():
                p.copy_(_tensor(z["mlp." + n], dev))
                st = {m: _tensor(z["mlp.%s.%s" % (m, n)], dev if m != "step" else "cpu") for m in ("exp_avg", "exp_avg_sq", "step")
                      if "mlp.%s.%s" % (m, n) in z.files}
                if st:
                    session.mlp_optimizer.state[p] = st
    pos, has_gauss = (int(v) for v in z["rng.np_pos"])
    np.random.set_state(("MT19937", z["rng.np_keys"], pos, has_gauss, float(z["rng.np_gauss"])))
    torch.set_rng_state(torch.from_numpy(np.ascontiguousarray(z["rng.torch"])))
    if "rng.torch_device" in z.files and dev.type == "cuda":
        torch.cuda.set_rng_state(torch.from_numpy(np.ascontiguousarray(z["rng.torch_device"])), dev)
    return t + 1


def _load_reference_checkpoint(session, directory, t, frames, dev):
    """scripts/hierslam.py:1717-1750 on frames(i); two deviations: the keyframe index list is cut to the entries < t,
    since frame t is stepped again and would be listed twice, and a keyframe keeps its label planes where its frame has them"""
    from . import slam
    if frames is None:
        raise RuntimeError("hsr_utils.checkpoint: %s has no session%d.npz beside it: a checkpoint of the reference's kind needs "
                           "frames=, a function from a frame index to its frame dict" % (directory, t))
    if t < 1:
        raise ValueError("hsr_utils.checkpoint: a checkpoint of the reference's kind resumes AT frame t, and frame 0 builds the map: "
                         "step a fresh session instead of loading time_idx %d" % t)
    session.initialize(frames(0))      # the reference initialises before it loads (:1690-1698): scene_radius, the leaf head
    session.params = _load_params(os.path.join(directory, "params%d.npz" % t), dev)
    P = session.params['means3D'].shape[0]
    for k in BOOKKEEPING:              # :1723-1726
        session.variables[k] = torch.zeros(P, dtype=torch.float32, device=dev)
    listed = np.load(os.path.join(directory, "keyframe_time_indices%d.npy" % t), allow_pickle=False).tolist()
    session.keyframe_time_indices = [int(i) for i in listed if int(i) < t]
    session.keyframe_list, session.gt_w2c_all_frames = [], []
    scale = session._png_depth_scale()
    packed = session.keyframe_store == "packed"
    for i in range(t):
        frame = frames(i)
        session.gt_w2c_all_frames.append(frame.get('gt_w2c'))
        if i in session.keyframe_time_indices:
            kf = {'id': i, 'est_w2c': slam.frame_w2c(session.params, i)}
            labels = frame.get('semantic_label_gt') if session.flag_use_semantic else None
            if packed:
                kf['packed'] = pack_keyframe(frame['im'], frame['depth'], labels, scale)
            else:
                kf['color'], kf['depth'] = frame['im'], frame['depth']
                if session.flag_use_semantic:
                    kf['label_gt'] = labels
            kf['cam'], kf['intrinsics'] = session.cam, session.intrinsics
            session.keyframe_list.append(kf)
    return t


__all__ = ["PackedKeyframe", "pack_keyframe", "unpack_keyframe", "raw_keyframe", "keyframe_planes", "save_checkpoint", "load_checkpoint"]
