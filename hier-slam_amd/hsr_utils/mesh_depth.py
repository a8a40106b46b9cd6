"""Depth images of a triangle mesh from given views, on the device (include/recon/hsr_mesh_depth.h), and the number
the reference family reports from them: Depth L1 of a run's mesh against the ground-truth mesh, both rendered from views the sensor never
took.  The header states the rule of the image; there the family leaves the device for Open3D.

    MeshDepthRenderer(vertices, faces, H, W)                    keeps the device mesh and the scratch of hsr_mesh_depth
        .render(w2c, intrinsics, near=0.01)                     (depth float32 [H,W], face int32 [H,W]): ONE hsr_mesh_depth, no host read
    render_mesh_depth(vertices, faces, w2c, intrinsics, H, W, near=0.01)      the one-shot form
    virtual_views(w2cs, targets, n, seed=0)                     float32 [n,4,4]: at the centres of given poses, looking at given points; host
    mesh_depth_l1(rec, gt, w2cs, intrinsics, H, W, near=0.01)   both meshes from every view; float64 sums on the device, ONE host read

There is no CPU path for anything that launches; virtual_views is host arithmetic in float64.
"""
import numpy as np
import torch

from diff_gaussian_rasterization import _abi
from .mesh_eval import MAX_IMAGE_SIDE, _device_tensor, _host

_lib = _abi.lib

SMALL_BOX = 255     # HSR_MESH_DEPTH_SMALL_BOX
_GOLDEN = 0x9E3779B97F4A7C15
_MASK = 2 ** 64 - 1


def _size(H, W):
    H, W = int(H), int(W)
    if not (1 <= H <= MAX_IMAGE_SIDE and 1 <= W <= MAX_IMAGE_SIDE):
        raise ValueError("hsr_utils.mesh_depth: the image is %d x %d; sides are 1..%d" % (W, H, MAX_IMAGE_SIDE))
    return H, W


def _pinhole(intrinsics):
    k = np.asarray(_host(intrinsics), dtype=np.float64)
    if k.ndim != 2 or k.shape[0] < 3 or k.shape[1] < 3:
        raise RuntimeError("hsr_utils.mesh_depth: intrinsics must be [3,3] (got %s)" % (k.shape,))
    return float(k[0][0]), float(k[1][1]), float(k[0][2]), float(k[1][2])


def _views(w2cs):
    views = np.ascontiguousarray(_host(w2cs), dtype=np.float32)
    if views.ndim != 3 or views.shape[1:] != (4, 4):
        raise RuntimeError("hsr_utils.mesh_depth: w2cs must be [T,4,4] (got %s)" % (views.shape,))
    return views


class MeshDepthRenderer:
    """The mesh (vertices float32 [V,3], faces int32 [F,3] on a HIP device; copies are made once) and the scratch for images of H x W.
    A RuntimeError names a vertices or faces that is not on the device: there is no CPU path.  ValueError on a mesh without vertices."""

    def __init__(self, vertices, faces, H, W):
        self.H, self.W = _size(H, W)
        self.vertices = _device_tensor(vertices, "vertices", torch.float32, 3)
        self.faces = _device_tensor(faces, "faces", torch.int32, 3, self.vertices.device)
        if self.vertices.shape[0] == 0:
            raise ValueError("hsr_utils.mesh_depth: the mesh has no vertices")
        self.device = self.vertices.device
        self.scratch_bytes = int(_lib.hsr_mesh_depth_scratch_bytes(self.faces.shape[0], self.H, self.W))
        self.scratch = torch.empty(self.scratch_bytes, dtype=torch.uint8, device=self.device)      # the allocator aligns to 256 bytes and more

    def render(self, w2c, intrinsics, near=0.01):
        """(depth float32 [H,W], face int32 [H,W]) on the device from the world-to-camera matrix w2c [4,4] (host or device: one copy of 16
        numbers to the host, by value into the launch) and intrinsics [3,3]: the depth along the camera's axis of the nearest face under
        every pixel centre and that face's index; 0 and -1 where there is none.  Nothing is read back."""
        near = float(near)
        if not (np.isfinite(near) and near > 0):
            raise ValueError("hsr_utils.mesh_depth: near must be finite and positive (got %r)" % near)
        m = np.ascontiguousarray(_host(w2c), dtype=np.float32)
        if m.shape != (4, 4):
            raise RuntimeError("hsr_utils.mesh_depth: w2c must be [4,4] (got %s)" % (m.shape,))
        fx, fy, cx, cy = _pinhole(intrinsics)
        depth = torch.empty((self.H, self.W), dtype=torch.float32, device=self.device)
        face = torch.empty((self.H, self.W), dtype=torch.int32, device=self.device)
        _abi.call(_lib.hsr_mesh_depth, "hsr_mesh_depth", self.device, self.vertices.shape[0], self.faces.shape[0], self.vertices.data_ptr(),
                  self.faces.data_ptr(), self.H, self.W, fx, fy, cx, cy, m.ctypes.data_as(_abi.fp), near, self.scratch.data_ptr(),
                  self.scratch_bytes, depth.data_ptr(), face.data_ptr())
        return depth, face


def render_mesh_depth(vertices, faces, w2c, intrinsics, H, W, near=0.01):
    """MeshDepthRenderer(vertices, faces, H, W).render(w2c, intrinsics, near): one image of a mesh that is rendered once"""
    return MeshDepthRenderer(vertices, faces, H, W).render(w2c, intrinsics, near)


def _splitmix(seed, n):
    """the n-th 64-bit word of include/eval/hsr_mesh_eval.h (hsr_mesh_sample)"""
    z = (seed + n * _GOLDEN) & _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


def virtual_views(w2cs, targets, n, seed=0):
    """n world-to-camera matrices, float32 [n,4,4] (numpy), of views the sensor never took: each stands where one of the given poses
    w2cs [T,4,4] stood — free space by construction, so no view is ever rejected — and looks at one of targets [M,3].  Host arithmetic
    in float64, the same views for the same seed.  The construction, for view i:
        z_k = the splitmix64 word of hsr_mesh_eval.h from seed + (3 * i + k + 1) * 0x9E3779B97F4A7C15        (k = 0, 1; k = 2 is not used)
        pose = w2cs[z_0 % T] with rotation R (rows: the image-right, image-down and viewing axes in the world) and translation t
        c = -R^T t, the camera centre;  p = targets[z_1 % M];  d = p - c
        |d| < 1e-6: the view is the pose itself.  Otherwise f = d / |d|, and with the hint h = R[1] (the pose's own image-down axis):
            |f x h| >= 1e-3:  right = (h x f) / |h x f|,  down = f x right
            else, with h = R[0] (its image-right axis):  down = (f x h) / |f x h|,  right = down x f
        the view's rotation has the rows right, down, f, and its translation is -(that rotation) c.
    targets may be a device tensor: only the n chosen rows are copied to the host."""
    poses = np.asarray(_host(w2cs), dtype=np.float64)
    n = int(n)
    if poses.ndim != 3 or poses.shape[1:] != (4, 4) or poses.shape[0] < 1:
        raise RuntimeError("hsr_utils.mesh_depth: w2cs must be [T,4,4] with T >= 1 (got %s)" % (poses.shape,))
    if n < 0:
        raise ValueError("hsr_utils.mesh_depth: the number of views must be >= 0 (got %d)" % n)
    shape = tuple(targets.shape) if hasattr(targets, "shape") else np.shape(targets)
    if len(shape) != 2 or shape[0] < 1 or shape[1] != 3:
        raise RuntimeError("hsr_utils.mesh_depth: targets must be [M,3] with M >= 1 (got %s)" % (shape,))
    T, M = poses.shape[0], shape[0]
    seed = int(seed) % 2 ** 64
    words = [(_splitmix(seed, 3 * i + 1), _splitmix(seed, 3 * i + 2)) for i in range(n)]
    rows = [z1 % M for _z0, z1 in words]
    if isinstance(targets, torch.Tensor):
        chosen = targets.detach()[torch.as_tensor(rows, dtype=torch.int64, device=targets.device)].cpu().numpy().astype(np.float64)
    else:
        chosen = np.asarray(targets, dtype=np.float64)[rows].reshape(n, 3)
    out = np.zeros((n, 4, 4), np.float32)
    for i, (z0, _z1) in enumerate(words):
        pose = poses[z0 % T]
        R, t = pose[:3, :3], pose[:3, 3]
        c = -R.T @ t
        d = chosen[i] - c
        length = np.linalg.norm(d)
        if not length >= 1e-6:
            out[i] = pose
            continue
        f = d / length
        side = np.cross(R[1], f)
        if np.linalg.norm(np.cross(f, R[1])) >= 1e-3:
            right = side / np.linalg.norm(side)
            down = np.cross(f, right)
        else:
            down = np.cross(f, R[0])
            down = down / np.linalg.norm(down)
            right = np.cross(down, f)
        view = np.eye(4)
        view[:3, :3] = np.stack([right, down, f])
        view[:3, 3] = -view[:3, :3] @ c
        out[i] = view
    return out


def mesh_depth_l1(rec, gt, w2cs, intrinsics, H, W, near=0.01):
    """Depth L1 of a reconstructed mesh against a ground-truth one, both (vertices, faces) in one world frame, from the views w2cs
    [T,4,4]: R and G are the two depth images of a view (MeshDepthRenderer.render), 0 where the mesh is not hit.  Returns
        depth_l1           the mean of |G - R| over all T * H * W pixels, with 0 where a mesh is not hit: the family's number, whose
                           renderers leave the background at 0 as well
        depth_l1_covered   the same mean over the pixels BOTH meshes hit; NaN when there are none
        gt_cover, rec_cover, both_cover      the shares of pixels the ground truth, the reconstruction and both hit
        per_view_l1        float64 [T] (numpy): depth_l1 of each view
    The sums accumulate on the device in float64; ONE host read at the end."""
    H, W = _size(H, W)
    views = _views(w2cs)
    dev = None
    for m in (rec[0], gt[0]):
        if isinstance(m, torch.Tensor) and m.is_cuda:
            dev = m.device
            break
    if dev is None:
        raise RuntimeError("hsr_utils.mesh_depth: the vertices of rec or gt must be a tensor on a HIP device; there is no CPU path")
    r = MeshDepthRenderer(_device_tensor(rec[0], "rec vertices", torch.float32, 3, dev), _device_tensor(rec[1], "rec faces", torch.int32, 3, dev), H, W)
    g = MeshDepthRenderer(_device_tensor(gt[0], "gt vertices", torch.float32, 3, dev), _device_tensor(gt[1], "gt faces", torch.int32, 3, dev), H, W)
    T = views.shape[0]
    sums = torch.zeros((T, 5), dtype=torch.float64, device=dev)      # |G - R| over all, over both, and the three counts
    for t, m in enumerate(views):
        R, rf = r.render(m, intrinsics, near)
        G, gf = g.render(m, intrinsics, near)
        diff = (G.double() - R.double()).abs()
        hit_r, hit_g = rf >= 0, gf >= 0
        both = hit_r & hit_g
        sums[t] = torch.stack([diff.sum(), (diff * both).sum(), hit_g.sum().double(), hit_r.sum().double(), both.sum().double()])
    s = sums.cpu().numpy()      # the one host read
    pixels = float(H * W)
    total = s.sum(axis=0) if T else np.zeros(5)
    n = max(T, 1) * pixels
    return dict(depth_l1=float(total[0] / n), depth_l1_covered=float(total[1] / total[4]) if total[4] > 0 else float("nan"),
                gt_cover=float(total[2] / n), rec_cover=float(total[3] / n), both_cover=float(total[4] / n), per_view_l1=s[:, 0] / pixels)


__all__ = ["MeshDepthRenderer", "render_mesh_depth", "virtual_views", "mesh_depth_l1"]
