"""The mesh of a finished run, on the device (include/ext/hsr_tsdf.h): the rendered depth of the finished map fused
into a truncated signed distance volume, one launch per view, and the volume's zero surface as a triangle mesh by marching tetrahedra.
What the reference family does with Open3D's TSDF integration after a run; the reference itself has no mesher, so the rules are this
project's own and the header states each of them.

    TsdfVolume(origin, dims, voxel_size, trunc=None, max_weight=64.0, color=True, labels=False, device="cuda")
        .integrate(depth, w2c, intrinsics, color=None, labels=None, opacity=None, sil_thres=None, depth_max=0.0)   ONE hsr_tsdf_integrate
        .extract()     hsr_tsdf_count, torch.cumsum, ONE host read (the triangle count), hsr_tsdf_faces, torch.unique, hsr_tsdf_vertices
    mesh_bounds(params, pad, voxel_size, max_voxels=2**28)    (origin, dims) of the padded box of the finite means3D
    save_mesh_ply(path, vertices, faces, rgb=None, labels=None), load_mesh_ply(path)
    mesh_run(params, out_path, voxel_size=, every=5, semantic=False, ...)    render every `every`-th pose, fuse, extract, save; with
        min_component_faces=, min_component_ratio= or largest_component= the small components are dropped first (mesh_clean.py)

There is no CPU path for anything that launches; the bounds and the file helpers are plain torch / numpy and run anywhere.
"""
import numpy as np
import torch

from diff_gaussian_rasterization import _abi

_lib = _abi.lib

MAX_IMAGE_SIDE = 16384      # HSR_TSDF_MAX_IMAGE_SIDE
MAX_POINTS = 2 ** 31 - 1
DEFAULT_MAX_VOXELS = 2 ** 28      # 28 bytes of full state per point: 7.5 GB
LABEL_MODES = ("flat", "tree", "leaf")


def _host(m):
    return m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)


def _p(t):
    return None if t is None else t.data_ptr()


class TsdfVolume:
    """An X x Y x Z grid of sample points (dims = (X, Y, Z), x fastest), point (i, j, k) at origin + voxel_size * (i, j, k), and its
    state as device tensors: .tsdf (1), .weight (0), with color=True .color [3,Z,Y,X] (0) and .cweight (0), with labels=True .best (+inf)
    and .label (int32, -1); the others float32 [Z,Y,X].  trunc defaults to 4 * voxel_size."""

    def __init__(self, origin, dims, voxel_size, trunc=None, max_weight=64.0, color=True, labels=False, device="cuda"):
        X, Y, Z = (int(d) for d in dims)
        if min(X, Y, Z) < 1 or X * Y * Z > MAX_POINTS:
            raise ValueError("hsr_utils.mesh: dims %s must be at least 1 a side and X*Y*Z <= 2^31-1" % ((X, Y, Z),))
        h = float(voxel_size)
        trunc = 4.0 * h if trunc is None else float(trunc)
        for name, v in (("voxel_size", h), ("trunc", trunc), ("max_weight", float(max_weight))):
            if not (np.isfinite(v) and v > 0):
                raise ValueError("hsr_utils.mesh: %s must be finite and positive (got %r)" % (name, v))
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("hsr_utils.mesh: the volume lives on a HIP device (got %s); there is no CPU path" % (dev,))
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.dims, self.origin = (X, Y, Z), tuple(float(o) for o in origin)
        self.voxel_size, self.trunc, self.max_weight, self.device = h, trunc, float(max_weight), dev
        f = dict(dtype=torch.float32, device=dev)
        self.tsdf, self.weight = torch.ones((Z, Y, X), **f), torch.zeros((Z, Y, X), **f)
        self.color, self.cweight = (torch.zeros((3, Z, Y, X), **f), torch.zeros((Z, Y, X), **f)) if color else (None, None)
        self.best, self.label = ((torch.full((Z, Y, X), float("inf"), **f), torch.full((Z, Y, X), -1, dtype=torch.int32, device=dev))
                                 if labels else (None, None))

    def _plane(self, t, what, H, W, dtype=torch.float32, lead=None):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("hsr_utils.mesh: %s must be a tensor on a HIP device; there is no CPU path" % what)
        if t.device != self.device:
            raise RuntimeError("hsr_utils.mesh: %s is on %s, the volume on %s" % (what, t.device, self.device))
        if t.dtype != dtype:
            raise RuntimeError("hsr_utils.mesh: %s must be %s (got %s)" % (what, dtype, t.dtype))
        want = (H, W) if lead is None else (lead, H, W)
        if tuple(t.shape[-len(want):]) != want or t.numel() != int(np.prod(want)):
            raise RuntimeError("hsr_utils.mesh: %s must be %s (got %s)" % (what, list(want), tuple(t.shape)))
        return t.detach().contiguous()

    def integrate(self, depth, w2c, intrinsics, color=None, labels=None, opacity=None, sil_thres=None, depth_max=0.0):
        """One view into the volume, ONE launch and no host read when w2c and intrinsics are on the host.  depth: float32 [H,W] or
        [1,H,W], z along the camera's axis; w2c [4,4] world-to-camera of the volume's frame; intrinsics [3,3].  color: float32 [3,H,W],
        fused where |sdf| <= trunc (needs color=True); labels: an integer plane [H,W] (int64, or int32 as evaluate.semantic_labels
        gives), the label of the view that saw the point closest to the surface (needs labels=True); opacity with sil_thres: only pixels
        whose opacity exceeds it count; depth_max > 0: deeper pixels do not."""
        if not isinstance(depth, torch.Tensor) or depth.dim() < 2:
            raise RuntimeError("hsr_utils.mesh: depth must be a tensor [H,W] or [1,H,W]")
        H, W = int(depth.shape[-2]), int(depth.shape[-1])
        if not (1 <= H <= MAX_IMAGE_SIDE and 1 <= W <= MAX_IMAGE_SIDE):
            raise ValueError("hsr_utils.mesh: the image is %d x %d; sides are 1..%d" % (W, H, MAX_IMAGE_SIDE))
        depth = self._plane(depth, "depth", H, W)
        if color is not None:
            if self.color is None:
                raise RuntimeError("hsr_utils.mesh: a colour image needs a volume made with color=True")
            color = self._plane(color, "color", H, W, lead=3)
        if labels is not None:
            if self.label is None:
                raise RuntimeError("hsr_utils.mesh: a label plane needs a volume made with labels=True")
            if isinstance(labels, torch.Tensor) and labels.dtype == torch.int32:
                labels = labels.to(torch.int64)
            labels = self._plane(labels, "labels", H, W, dtype=torch.int64)
        if (opacity is None) != (sil_thres is None):
            raise ValueError("hsr_utils.mesh: opacity and sil_thres come together")
        if opacity is not None:
            opacity = self._plane(opacity, "opacity", H, W)
        m = np.ascontiguousarray(_host(w2c), dtype=np.float32)
        k = _host(intrinsics)
        if m.shape != (4, 4) or k.ndim != 2 or k.shape[0] < 3 or k.shape[1] < 3:
            raise RuntimeError("hsr_utils.mesh: w2c must be [4,4] and intrinsics [3,3] (got %s and %s)" % (m.shape, k.shape))
        X, Y, Z = self.dims
        _abi.call(_lib.hsr_tsdf_integrate, "hsr_tsdf_integrate", self.device, X, Y, Z, *self.origin, self.voxel_size, self.trunc, self.max_weight,
                  H, W, float(k[0][0]), float(k[1][1]), float(k[0][2]), float(k[1][2]), m.ctypes.data_as(_abi.fp), depth.data_ptr(), _p(color),
                  _p(labels), _p(opacity), 0.0 if sil_thres is None else float(sil_thres), float(depth_max), self.tsdf.data_ptr(),
                  self.weight.data_ptr(), _p(self.color), _p(self.cweight), _p(self.best), _p(self.label))
        return self

    def extract(self):
        """(vertices float32 [V,3], faces int32 [F,3], rgb uint8 [V,3] | None, labels int32 [V] | None) on the device: the zero
        surface over the cubes whose eight points were all observed.  Vertices are ordered by their edge key and the faces are emitted
        cube by cube, so two calls give identical tensors.  Empty tensors of those shapes when there is no surface."""
        X, Y, Z = self.dims
        dev = self.device
        counts = torch.empty(X * Y * Z, dtype=torch.int32, device=dev)
        _abi.call(_lib.hsr_tsdf_count, "hsr_tsdf_count", dev, X, Y, Z, self.tsdf.data_ptr(), self.weight.data_ptr(), counts.data_ptr())
        offsets = torch.cumsum(counts, 0, dtype=torch.int64)
        T = int(offsets[-1])      # the one host read
        keys = torch.empty((T, 3), dtype=torch.int64, device=dev)
        _abi.call(_lib.hsr_tsdf_faces, "hsr_tsdf_faces", dev, X, Y, Z, self.tsdf.data_ptr(), self.weight.data_ptr(), offsets.data_ptr(), T,
                  keys.data_ptr() if T else None)
        del counts, offsets
        vkeys, inverse = torch.unique(keys, return_inverse=True)      # sorted
        faces = inverse.reshape(T, 3).to(torch.int32)
        V = int(vkeys.numel())
        vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
        rgb = None if self.color is None else torch.empty((V, 3), dtype=torch.uint8, device=dev)
        labels = None if self.label is None else torch.empty((V,), dtype=torch.int32, device=dev)
        _abi.call(_lib.hsr_tsdf_vertices, "hsr_tsdf_vertices", dev, X, Y, Z, *self.origin, self.voxel_size, V, vkeys.data_ptr() if V else None,
                  self.tsdf.data_ptr(), _p(self.color), _p(self.cweight), _p(self.label), vertices.data_ptr() if V else None,
                  None if rgb is None or V == 0 else rgb.data_ptr(), None if labels is None or V == 0 else labels.data_ptr())
        return vertices, faces, rgb, labels


def mesh_bounds(params, pad, voxel_size, max_voxels=DEFAULT_MAX_VOXELS):
    """(origin, dims) of a volume around a map: the axis-aligned box of the finite rows of params['means3D'], grown by `pad` on every
    side, sampled every voxel_size (dims = ceil(extent / voxel_size) + 1 points a side).  ValueError when that is more than max_voxels
    points (the default 2^28 is 7.5 GB of full state); the message names a voxel size that fits.  One host read of six numbers."""
    h, pad = float(voxel_size), float(pad)
    if not (np.isfinite(h) and h > 0) or not (np.isfinite(pad) and pad >= 0):
        raise ValueError("hsr_utils.mesh: voxel_size must be finite and positive and pad finite and not negative (got %r and %r)" % (h, pad))
    means = params['means3D']
    means = means.detach() if isinstance(means, torch.Tensor) else torch.as_tensor(np.asarray(means))
    means = means[torch.isfinite(means).all(dim=1)].to(torch.float32)
    if means.shape[0] == 0:
        raise ValueError("hsr_utils.mesh: the map has no finite means3D")
    box = torch.stack([means.min(dim=0).values, means.max(dim=0).values]).cpu().numpy().astype(np.float64)
    lo, extent = box[0] - pad, (box[1] - box[0]) + 2 * pad

    def sides(step):
        return [int(np.ceil(e / step)) + 1 for e in extent]

    dims = sides(h)
    if int(np.prod([float(d) for d in dims])) > int(max_voxels):
        fit = max(h, float(np.cbrt(np.prod(np.maximum(extent, h)) / float(max_voxels))))
        while np.prod([float(d) for d in sides(fit)]) > int(max_voxels):
            fit *= 1.02
        raise ValueError("hsr_utils.mesh: a voxel size of %g gives %d x %d x %d = %d points, more than max_voxels = %d; a voxel size of "
                         "%.4g fits" % (h, dims[0], dims[1], dims[2], int(np.prod([float(d) for d in dims])), int(max_voxels), fit))
    return tuple(float(np.float32(v)) for v in lo), tuple(dims)


# ---- the file -----------------------------------------------------------------------------------------------------------------------------
def _vertex_dtype(rgb, labels):
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if rgb:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    if labels:
        fields += [("label", "<i4")]
    return np.dtype(fields)


_FACE = np.dtype([("n", "u1"), ("vertex_indices", "<i4", (3,))])
_PLY_NAMES = {"<f4": "float", "u1": "uchar", "|u1": "uchar", "<i4": "int"}


def save_mesh_ply(path, vertices, faces, rgb=None, labels=None):
    """a binary little-endian PLY: vertex x y z (float), with rgb red green blue (uchar), with labels label (int); face
    `property list uchar int vertex_indices`.  Tensors (one device-to-host copy each) or arrays.  Returns the path."""
    v = np.ascontiguousarray(_host(vertices), dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(_host(faces), dtype=np.int32).reshape(-1, 3)
    vd = _vertex_dtype(rgb is not None, labels is not None)
    vert = np.empty(v.shape[0], vd)
    vert["x"], vert["y"], vert["z"] = v[:, 0], v[:, 1], v[:, 2]
    if rgb is not None:
        c = np.asarray(_host(rgb)).reshape(-1, 3)
        if c.dtype != np.uint8 or c.shape[0] != v.shape[0]:
            raise RuntimeError("hsr_utils.mesh: rgb must be uint8 [V,3] (got %s %s)" % (c.dtype, c.shape))
        vert["red"], vert["green"], vert["blue"] = c[:, 0], c[:, 1], c[:, 2]
    if labels is not None:
        lab = np.asarray(_host(labels)).reshape(-1)
        if lab.shape[0] != v.shape[0]:
            raise RuntimeError("hsr_utils.mesh: labels must be [V] (got %s)" % (lab.shape,))
        vert["label"] = lab.astype(np.int32)
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise RuntimeError("hsr_utils.mesh: a face index is outside 0..%d" % (v.shape[0] - 1))
    face = np.empty(f.shape[0], _FACE)
    face["n"], face["vertex_indices"] = 3, f
    lines = ["ply", "format binary_little_endian 1.0", "element vertex %d" % v.shape[0]]
    lines += ["property %s %s" % (_PLY_NAMES[vd.fields[n][0].str], n) for n in vd.names]
    lines += ["element face %d" % f.shape[0], "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(lines) + "\n").encode("ascii"))
        out.write(vert.tobytes())
        out.write(face.tobytes())
    return path


def load_mesh_ply(path):
    """(vertices float32 [V,3], faces int32 [F,3], rgb uint8 [V,3] | None, labels int32 [V] | None) of a file save_mesh_ply wrote"""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("hsr_utils.mesh: %s is not a binary little-endian PLY" % path)
    counts, names, element = {}, [], None
    for line in lines[2:]:
        tok = line.split()
        if tok[:1] == ["element"]:
            element, counts[tok[1]] = tok[1], int(tok[2])
        elif tok[:1] == ["property"] and element == "vertex":
            names.append(tok[2])
        elif tok[:1] == ["property"] and tok[1:] != ["list", "uchar", "int", "vertex_indices"]:
            raise ValueError("hsr_utils.mesh: unknown face property %r" % line)
    vd = _vertex_dtype("red" in names, "label" in names)
    if list(vd.names) != names:
        raise ValueError("hsr_utils.mesh: unknown vertex layout %s" % names)
    V, F = counts.get("vertex", 0), counts.get("face", 0)
    vert = np.frombuffer(data, vd, V, end)
    face = np.frombuffer(data, _FACE, F, end + V * vd.itemsize)
    if len(data) != end + V * vd.itemsize + F * _FACE.itemsize or (F and (face["n"] != 3).any()):
        raise ValueError("hsr_utils.mesh: %s does not hold %d vertices and %d triangles" % (path, V, F))
    xyz = np.stack([vert["x"], vert["y"], vert["z"]], axis=1) if V else np.zeros((0, 3), np.float32)
    rgb = np.stack([vert["red"], vert["green"], vert["blue"]], axis=1) if "red" in names else None
    return xyz, np.ascontiguousarray(face["vertex_indices"]), rgb, (np.ascontiguousarray(vert["label"]) if "label" in names else None)


# ---- a run --------------------------------------------------------------------------------------------------------------------------------
def mesh_run(params, out_path, *, voxel_size, every=5, semantic=False, label_mode="flat", sil_thres=0.5, depth_max=0.0, bounds=None,
             intrinsics=None, width=None, height=None, num_frames=None, cam=None, first_frame_w2c=None, pad=None, trunc=None, max_weight=64.0,
             max_voxels=DEFAULT_MAX_VOXELS, near=0.01, far=100, level_sizes=None, tree_table=None, mlp=None, min_component_faces=0,
             min_component_ratio=0.0, largest_component=False):
    """The mesh of a finished run as a PLY file.  For every `every`-th step t the finished map `params` is rendered from the estimated
    pose of frame t (slam.render_params, without gradients) and the view is fused into a TsdfVolume: depth and colour where the final
    opacity exceeds sil_thres and, with semantic=True (the semantic rasterizer), the class plane of evaluate.semantic_labels(mode
    label_mode: "flat", "tree" with level_sizes and tree_table, or "leaf" with mlp).  Then extract and save_mesh_ply.  Nothing is read
    back inside the loop.  params is the dictionary of a finished run (map_io.load_params(path, device)); intrinsics, width, height,
    num_frames and first_frame_w2c default to its 'intrinsics', 'org_width', 'org_height', the number of pose columns and 'w2c' (else
    the identity); cam is the camera to render with (default: setup_camera of those).  bounds = (origin, dims) of the volume, default
    mesh_bounds(params, pad, voxel_size, max_voxels) with pad = trunc.  min_component_faces, min_component_ratio and largest_component
    are mesh_clean.clean_mesh's min_faces, min_ratio and largest: with one of them set, the small disconnected pieces of the mesh are
    dropped on the device between extract and save; with all three at their defaults clean_mesh is not called and the file is what it
    always was.  Returns (path, number of vertices, number of faces)."""
    from . import evaluate, slam
    from .camera import setup_camera
    from .replay import run_w2cs
    if int(every) < 1:
        raise ValueError("hsr_utils.mesh: every must be >= 1")
    if label_mode not in LABEL_MODES:
        raise ValueError("hsr_utils.mesh: label_mode must be one of %s (got %r)" % (", ".join(LABEL_MODES), label_mode))
    if semantic and 'semantic' not in params:
        raise RuntimeError("hsr_utils.mesh: semantic=True needs params['semantic']")
    h = float(voxel_size)
    trunc = 4.0 * h if trunc is None else float(trunc)
    k = np.asarray(_host(params['intrinsics'] if intrinsics is None else intrinsics), dtype=np.float32)[:3, :3]
    w = int(_host(params['org_width'])) if width is None else int(width)
    hgt = int(_host(params['org_height'])) if height is None else int(height)
    T = int(params['cam_unnorm_rots'].shape[-1]) if num_frames is None else int(num_frames)
    if first_frame_w2c is None:
        first_frame_w2c = params['w2c'] if 'w2c' in params else np.eye(4)
    first = np.asarray(_host(first_frame_w2c), dtype=np.float32)
    if first.shape != (4, 4):
        raise RuntimeError("hsr_utils.mesh: first_frame_w2c must be [4,4] (got %s)" % (first.shape,))
    origin, dims = mesh_bounds(params, trunc if pad is None else pad, h, max_voxels) if bounds is None else bounds
    dev = params['means3D'].device
    if cam is None:
        cam = setup_camera(w, hgt, k, first, near, far, device=dev)
    # the rendered depth is z in the frame of cam's view matrix applied after the frame's relative pose: one product per view, on the host
    views = run_w2cs(params).cpu().numpy()[:T]      # one copy for the run
    if not np.array_equal(first, np.eye(4, dtype=np.float32)):
        views = [first @ m for m in views]
    vol = TsdfVolume(origin, dims, h, trunc=trunc, max_weight=max_weight, color=True, labels=bool(semantic), device=dev)
    with torch.no_grad():
        for t in range(0, T, int(every)):
            _rv, im, _radius, sem, depth, opac = slam.render_params(params, t, cam, bool(semantic))
            labels = None
            if semantic:
                labels = evaluate.semantic_labels(sem, label_mode, level_sizes=level_sizes, tree_table=tree_table, mlp=mlp)
                labels = (labels[0] if label_mode == "tree" else labels).to(torch.int64)
            vol.integrate(depth, views[t], k, color=im, labels=labels, opacity=opac, sil_thres=sil_thres, depth_max=depth_max)
    vertices, faces, rgb, labels = vol.extract()
    if int(min_component_faces) != 0 or float(min_component_ratio) != 0.0 or largest_component:
        from . import mesh_clean
        vertices, faces, rgb, labels = mesh_clean.clean_mesh(vertices, faces, rgb, labels, min_faces=min_component_faces,
                                                             min_ratio=min_component_ratio, largest=bool(largest_component))
    save_mesh_ply(out_path, vertices, faces, rgb, labels)
    return out_path, int(vertices.shape[0]), int(faces.shape[0])


__all__ = ["TsdfVolume", "mesh_bounds", "save_mesh_ply", "load_mesh_ply", "mesh_run"]
