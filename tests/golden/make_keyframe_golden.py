"""Generates tests/golden/keyframes/*.npz: inputs and outputs of the reference's own keyframe_selection_overlap
(utils/keyframe_selection.py:40-96), imported from /root/reference in the build container and run on the CPU.  Its only device placement
is `torch.zeros((1, 3)).cuda()` (:29); torch.Tensor.cuda is the identity inside this process — placement only, the arithmetic is
untouched.  Intermediate values are observed, not recomputed: get_pointcloud is wrapped (its sampled pixels and its surviving points),
so are the module's view of sorted() (every keyframe's percent_inside) and of torch.matmul (the homogeneous image coordinates of :72).
Only data is stored.

Each scene is accepted only under the conditions of tests/keyframe_ref.py's borderline rule, all asserted here against the reference's
own fp32 values (see check()); a scene that breaks one is drawn again with the next seed, the bounds are never widened.
Run: python tests/golden/make_keyframe_golden.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")
import keyframe_ref as R  # noqa: E402
import utils.keyframe_selection as KS  # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self          # :29 — placement only

MAX_BORDERLINE_FRACTION = 5e-4                           # 0.05 % of all (point, keyframe) pairs


class Recorder:
    """Stands where the module looks up `torch`, `sorted` and get_pointcloud; records what passes through and changes nothing."""

    def __init__(self):
        self.matmul, self.percent, self.sampled, self.pts = [], None, None, None
        self._get_pointcloud = KS.get_pointcloud

    def record_matmul(self, a, b):
        out = torch.matmul(a, b)
        self.matmul.append(out.clone())
        return out

    def record_sorted(self, items, **kw):
        self.percent = np.array([float(i['percent_inside']) for i in items], dtype=np.float32)
        return sorted(items, **kw)

    def record_pointcloud(self, depth, intrinsics, w2c, sampled_indices):
        self.sampled = sampled_indices.clone()
        self.pts = self._get_pointcloud(depth, intrinsics, w2c, sampled_indices)
        return self.pts


def run_reference(depth, w2c, K, keyframes, k, pixels, torch_seed, numpy_seed):
    rec = Recorder()
    proxy = type("TorchView", (), {"__getattr__": lambda s, n: rec.record_matmul if n == "matmul" else getattr(torch, n)})()
    saved = KS.torch, KS.get_pointcloud
    KS.torch, KS.get_pointcloud, KS.sorted = proxy, rec.record_pointcloud, rec.record_sorted
    try:
        torch.manual_seed(torch_seed)
        np.random.seed(numpy_seed)
        selected = KS.keyframe_selection_overlap(depth, w2c, K, keyframes, k, pixels)
    finally:
        KS.torch, KS.get_pointcloud = saved
        del KS.sorted
    return rec, np.array(selected, dtype=np.int64)


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    x, y, z = axis
    Kx = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def pose(Rm, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm, t
    return T


def scene(g, H, W, n_kf, band):
    """A smooth depth in 1/256 steps (it compresses) with invalid holes and an empty band of rows; keyframes scattered around the
    current pose, of which one is the current pose itself and one looks the other way.  The keyframe at the current pose projects every
    point onto its own pixel centre, so the pixels of rows / columns EDGE and size - EDGE sit exactly on a threshold and are borderline by
    construction; `band` invalidates the outer EDGE + 1 pixels (a sensor's dead border) and with them those pairs."""
    yy, xx = np.mgrid[0:H, 0:W]
    a, b, c = g.uniform(0.5, 1.5, 3)
    depth = 2.5 + 0.8 * np.sin(a * 4 * xx / W + 1.0) + 0.6 * np.cos(b * 3 * yy / H) + 0.3 * np.sin(c * 5 * (xx + yy) / (W + H))
    depth = np.round(depth * 256) / 256
    for _ in range(6):
        y0, x0 = int(g.integers(0, H - 8)), int(g.integers(0, W - 8))
        depth[y0:y0 + int(g.integers(4, H // 4)), x0:x0 + int(g.integers(4, W // 4))] = 0.0
    r0 = int(g.integers(H // 4, H // 2))
    depth[r0:r0 + 3] = 0.0                                   # rows without a valid pixel
    depth[0, :] = 0.0
    if band:
        e = R.EDGE + 1
        depth[:e], depth[-e:], depth[:, :e], depth[:, -e:] = 0.0, 0.0, 0.0, 0.0
    K = np.array([[W / 2.0, 0, W / 2.0 - 0.5], [0, W / 2.0, H / 2.0 - 0.5], [0, 0, 1]])
    w2c = pose(rotation(g.normal(size=3), g.uniform(0.2, 0.6)), g.uniform(-0.5, 0.5, 3))
    kfs = []
    for i in range(n_kf):
        if i == 2:
            rel = np.eye(4)                                  # the current pose itself
        elif i == 5:
            rel = pose(rotation([0, 1, 0], np.pi), g.uniform(-0.1, 0.1, 3))     # facing away: sees nothing
        else:
            s = g.uniform(0.05, 1.0)
            rel = pose(rotation(g.normal(size=3), s * g.uniform(0.1, 1.2)), s * g.uniform(-1.2, 1.2, 3))
        kfs.append(rel @ w2c)
    f32 = lambda m: torch.tensor(np.asarray(m, np.float32))
    return f32(depth[None]), f32(w2c), f32(K), [f32(m) for m in kfs]


def check(depth, w2c, K, poses, rec, selected, k, numpy_seed):
    """The conditions a fixture must meet; returns (arrays to store, None) or (None, the reason it fails)."""
    H, W = depth.shape[1:]
    n_kf = poses.shape[0]
    sampled, pts_ref = rec.sampled, rec.pts
    # the removal step is unambiguous: removed = drawn more than once, or at the origin; no two different pixels with near-equal keys
    keep = torch.zeros(len(sampled), dtype=torch.bool)
    pts_all32 = R.back_project(depth, K, w2c, sampled)
    keep_rule = R.keep_by_pixels(sampled, pts_all32)
    if int(keep_rule.sum()) != pts_ref.shape[0] or not torch.equal(pts_all32[keep_rule], pts_ref):
        return None, "removed set is not (drawn twice | origin)"
    keep = keep_rule
    uniq_pix, first = np.unique(sampled.numpy(), axis=0, return_index=True)
    keys = R.round_key(pts_all32[torch.tensor(first)]).double()
    d = (keys[:, None, :] - keys[None, :, :]).abs().amax(dim=2)
    d.fill_diagonal_(1.0)
    if float(d.min()) <= 2e-4:
        return None, "two different pixels with keys within 2e-4"
    if int((~keep).sum()) == 0:
        return None, "no duplicated draw"
    # float64 chain from the inputs
    pts64 = R.back_project(depth, K, w2c, sampled, torch.float64)[keep]
    inside64, border, u64, v64, m = R.borderline(pts64, poses, K, W, H)
    # the reference's own fp32 coordinates: its matmul outputs (:72) through the element-wise lines :74-81
    p2d = torch.stack([x.transpose(0, 1) for x in rec.matmul])                         # [n_kf, n, 3]
    zz = p2d[:, :, 2:] + 1e-5
    uv = (p2d / zz)[:, :, :2]
    inside_ref = (uv[..., 0] < W - R.EDGE) & (uv[..., 0] > R.EDGE) & (uv[..., 1] < H - R.EDGE) & (uv[..., 1] > R.EDGE) & (zz[..., 0] > 0)
    counts_ref = inside_ref.sum(dim=1)
    if not np.array_equal((counts_ref / uv.shape[1]).numpy().astype(np.float32), rec.percent):
        return None, "percent_inside does not follow from the recorded coordinates"
    front = (zz[..., 0].double() > 0) & ~border
    err = torch.maximum((uv[..., 0].double() - u64).abs(), (uv[..., 1].double() - v64).abs())
    worst = float((err / m)[front].max()) if bool(front.any()) else 0.0
    if worst > 0.25:
        return None, "reference fp32 error %.3f m exceeds m/4" % worst
    if not torch.equal(inside_ref[~border], inside64[~border]):
        return None, "a decision off the borderline differs from float64"
    b = border.sum(dim=1).numpy().astype(np.int32)
    c = counts_ref.numpy().astype(np.int64)
    if b.sum() > MAX_BORDERLINE_FRACTION * border.numel():
        return None, "too many borderline pairs: %d" % b.sum()
    if not ((c == 0) & (b == 0)).any():
        return None, "no keyframe with count 0 and b 0"
    if ((c > 0) & (c <= b)).any() or ((c == 0) & (b > 0)).any():
        return None, "a count within b of zero"
    for i in range(n_kf):
        for j in range(i + 1, n_kf):
            if (b[i] or b[j]) and abs(c[i] - c[j]) <= b[i] + b[j]:
                return None, "keyframes %d and %d could swap" % (i, j)
    np.random.seed(numpy_seed)
    if not np.array_equal(np.random.permutation(np.array(R.selection_order(c)))[:k], selected):
        return None, "returned list does not follow from the counts"
    return {"sampled_pixels": sampled.numpy().astype(np.int32), "keep": keep.numpy().astype(np.uint8), "pts": pts_ref.numpy(),
            "percent_inside": rec.percent, "counts": c, "borderline": b, "selected": selected,
            "worst_ref_error_over_m": np.float64(worst)}, None


CASES = {   # name: H, W, keyframes, k, pixels, dead border, want no borderline pair at all
    "a_96x128": (96, 128, 12, 4, 250, True, True),
    "b_240x320": (240, 320, 24, 8, 1000, True, False),
    "c_340x600": (340, 600, 40, 18, 1600, False, False),
    "d_120x160_k_large": (120, 160, 10, 30, 400, True, False),
}


def main():
    out_dir = os.path.join(HERE, "keyframes")
    os.makedirs(out_dir, exist_ok=True)
    for idx, (name, (H, W, n_kf, k, pixels, band, want_clean)) in enumerate(CASES.items()):
        for attempt in range(200):
            scene_seed = 1000 * (idx + 1) + attempt
            torch_seed, numpy_seed = scene_seed + 7, scene_seed + 11
            depth, w2c, K, kfs = scene(np.random.default_rng(scene_seed), H, W, n_kf, band)
            rec, selected = run_reference(depth, w2c, K, [{'est_w2c': m} for m in kfs], k, pixels, torch_seed, numpy_seed)
            poses = torch.stack(kfs)
            arrays, why = check(depth, w2c, K, poses, rec, selected, k, numpy_seed)
            if arrays is not None and want_clean and arrays["borderline"].sum() != 0:
                arrays, why = None, "borderline pairs in the scene that wants none"
            if arrays is not None:
                break
            print("%s: seed %d rejected: %s" % (name, scene_seed, why))
        else:
            raise SystemExit("%s: no seed met the conditions" % name)
        arrays.update(depth=depth.numpy(), w2c=w2c.numpy(), intrinsics=K.numpy(), est_w2c=poses.numpy(), k=np.int32(k),
                      pixels=np.int32(pixels), torch_seed=np.int64(torch_seed), numpy_seed=np.int64(numpy_seed),
                      scene_seed=np.int64(scene_seed))
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, **arrays)
        print("%s: seed %d, %d of %d points survive, counts %s, borderline %d, selected %s, worst reference error %.3f m, %d bytes" % (
            name, scene_seed, arrays["pts"].shape[0], pixels, arrays["counts"].tolist(), arrays["borderline"].sum(),
            selected.tolist(), arrays["worst_ref_error_over_m"], os.path.getsize(path)))


if __name__ == "__main__":
    main()
