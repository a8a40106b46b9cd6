"""Pictures of a triangle mesh without a window, on the device (include/shade/hsr_mesh_shade.h): the figures the
reference family makes in Open3D's viewer — the shaded mesh, the mesh in vertex colours, in class colours, as a heat map of its error
against the ground truth — from a headless box.  The header states the rule of every byte.

    vertex_normals(vertices, faces)                              float32 [V,3]: area-weighted, the same bytes on every run; ONE hsr_mesh_normals
    MeshRenderer(vertices, faces, H, W, rgb=None, labels=None, normals="smooth")      keeps a MeshDepthRenderer and the normals
        .render(w2c, intrinsics, pictures=("shaded",), ...)      dict: depth, face and one uint8 [H,W,3] per picture: ONE hsr_mesh_depth
                                                                 and ONE hsr_mesh_shade, no host read
    vertex_errors(vertices, points, cell=None)                   float32 [V]: the distance to the nearest of points (NearestGrid)
    orbit_views(lo, hi, n, elevation_deg=30.0, distance=None, up=None)      float32 [n,4,4]: cameras on a circle round a box; host
    render_mesh_views(mesh, w2cs, intrinsics, H, W, out_dir=None, ...)      the pictures of every view, as tensors or as PNG files
    render_mesh_run(params, mesh, out_dir, every=50, orbit=0, ...)          from the estimated poses of a finished run and an orbit

There is no CPU path for anything that launches; orbit_views is host arithmetic in float64.
"""
import os

import numpy as np
import torch

from diff_gaussian_rasterization import _abi
from .mesh_depth import MeshDepthRenderer, _pinhole, _views
from .mesh_eval import _device_tensor, _host

_lib = _abi.lib

MAX_JOBS = 8                                              # HSR_SHADE_MAX_JOBS
SHADED, COLOUR, NORMALS, LABELS, SCALAR = 0, 1, 2, 3, 4      # HSR_SHADE_*
PICTURES = ("shaded", "colour", "normals", "labels", "scalar")
_KINDS = dict(zip(PICTURES, (SHADED, COLOUR, NORMALS, LABELS, SCALAR)))


def vertex_normals(vertices, faces):
    """float32 [V,3] on the device: the area-weighted normal of every vertex (the sum of cross(B - A, C - A) over its faces,
    normalised; zero for a vertex of no face), accumulated in 64-bit fixed point so that the result is the same bytes on every run.
    ONE hsr_mesh_normals; nothing is read back.  ValueError on a mesh without vertices."""
    v = _device_tensor(vertices, "vertices", torch.float32, 3)
    f = _device_tensor(faces, "faces", torch.int32, 3, v.device)
    if v.shape[0] == 0:
        raise ValueError("hsr_utils.mesh_view: the mesh has no vertices")
    size = int(_lib.hsr_mesh_normals_scratch_bytes(v.shape[0]))
    scratch = torch.empty(size, dtype=torch.uint8, device=v.device)      # the allocator aligns to 256 bytes and more
    out = torch.empty((v.shape[0], 3), dtype=torch.float32, device=v.device)
    _abi.call(_lib.hsr_mesh_normals, "hsr_mesh_normals", v.device, v.shape[0], f.shape[0], v.data_ptr(), f.data_ptr(), scratch.data_ptr(), size,
              out.data_ptr())
    return out


def _colour3(value, what):
    c = [int(x) for x in value]
    if len(c) != 3 or not all(0 <= x <= 255 for x in c):
        raise ValueError("hsr_utils.mesh_view: %s must be three integers in 0..255 (got %r)" % (what, value))
    return c


class MeshRenderer:
    """The mesh (vertices float32 [V,3], faces int32 [F,3] on a HIP device), its attributes (rgb uint8 [V,3], labels int32 [V], either
    may be None) and what pictures of H x W need: a MeshDepthRenderer and the shading normals — "smooth": vertex_normals, computed once
    here; "flat": the normal of the face under the pixel; or a float32 [V,3] tensor of world-space normals."""

    def __init__(self, vertices, faces, H, W, rgb=None, labels=None, normals="smooth"):
        self.depth = MeshDepthRenderer(vertices, faces, H, W)
        self.H, self.W, self.device = self.depth.H, self.depth.W, self.depth.device
        self.vertices, self.faces = self.depth.vertices, self.depth.faces
        V = self.vertices.shape[0]
        self.rgb = None if rgb is None else _device_tensor(rgb, "rgb", torch.uint8, 3, self.device)
        self.labels = None if labels is None else _device_tensor(labels, "labels", torch.int32, None, self.device)
        if isinstance(normals, str):
            if normals not in ("smooth", "flat"):
                raise ValueError("hsr_utils.mesh_view: normals must be \"smooth\", \"flat\" or a [V,3] tensor (got %r)" % normals)
            self.normals = vertex_normals(self.vertices, self.faces) if normals == "smooth" else None
        else:
            self.normals = _device_tensor(normals, "normals", torch.float32, 3, self.device)
        for name, t in (("rgb", self.rgb), ("labels", self.labels), ("normals", self.normals)):
            if t is not None and t.shape[0] != V:
                raise RuntimeError("hsr_utils.mesh_view: %s must have %d rows, one a vertex (got %s)" % (name, V, tuple(t.shape)))

    def render(self, w2c, intrinsics, pictures=("shaded",), near=0.01, ambient=0.25, albedo=(0.8, 0.8, 0.8), background=(255, 255, 255),
               label_table=None, scalar=None, scalar_range=None, scalar_table=None, lit=True):
        """{"depth": float32 [H,W], "face": int32 [H,W], picture: uint8 [H,W,3] (R, G, B) for every name in pictures} on the device,
        from the world-to-camera matrix w2c [4,4] and intrinsics [3,3].  The pictures:
            "shaded"    albedo times the headlight's shade = ambient + (1 - ambient) * |n . v|
            "colour"    the vertex colours (rgb), interpolated; times the shade when lit
            "normals"   the shading normal in camera space as a colour; a surface that faces the camera is blue
            "labels"    the label of the nearest corner through label_table uint8 [n,3] (default label_colormap(256)); lit or not
            "scalar"    scalar float32 [V], interpolated, through scalar_table uint8 [256,3] (default jet_colormap) between
                        scalar_range = (lo, hi); lit or not
        Pixels no face covers get `background`.  ONE hsr_mesh_depth and ONE hsr_mesh_shade; nothing is read back: scalar_range
        is therefore required with "scalar"."""
        pictures = (pictures,) if isinstance(pictures, str) else tuple(pictures)
        if not 1 <= len(pictures) <= MAX_JOBS or len(set(pictures)) != len(pictures) or any(p not in PICTURES for p in pictures):
            raise ValueError("hsr_utils.mesh_view: pictures must be 1..%d different names of %s (got %r)" % (MAX_JOBS, ", ".join(PICTURES), pictures))
        ambient = float(ambient)
        if not 0.0 <= ambient <= 1.0:
            raise ValueError("hsr_utils.mesh_view: ambient must be in [0, 1] (got %r)" % ambient)
        bg = _colour3(background, "background")
        keep = []      # what the job structs point to, alive until the launch is enqueued
        jobs = (_abi.hsr_shade_job * len(pictures))()
        out = {}
        for job, name in zip(jobs, pictures):
            job.kind, job.lit, job.ambient = _KINDS[name], int(bool(lit)), ambient
            job.normals = None if self.normals is None else self.normals.data_ptr()
            job.albedo[:] = [float(a) for a in albedo]
            job.background[:] = bg + [0]
            if name == "colour":
                if self.rgb is None:
                    raise RuntimeError("hsr_utils.mesh_view: the \"colour\" picture needs the mesh's rgb")
                job.attr = self.rgb.data_ptr()
            elif name == "labels":
                if self.labels is None:
                    raise RuntimeError("hsr_utils.mesh_view: the \"labels\" picture needs the mesh's labels")
                table = label_table
                if table is None:
                    from .export import label_colormap
                    table = label_colormap(256, self.device)
                table = _device_tensor(table, "label_table", torch.uint8, 3, self.device)
                keep.append(table)
                job.attr, job.table, job.n = self.labels.data_ptr(), table.data_ptr(), table.shape[0]
            elif name == "scalar":
                if scalar is None or scalar_range is None:
                    raise RuntimeError("hsr_utils.mesh_view: the \"scalar\" picture needs scalar [V] and scalar_range (lo, hi)")
                values = _device_tensor(scalar, "scalar", torch.float32, None, self.device)
                if values.shape[0] != self.vertices.shape[0]:
                    raise RuntimeError("hsr_utils.mesh_view: scalar must be [V] = [%d] (got %s)" % (self.vertices.shape[0], tuple(values.shape)))
                table = scalar_table
                if table is None:
                    from .export import jet_colormap
                    table = jet_colormap(self.device)
                table = _device_tensor(table, "scalar_table", torch.uint8, 3, self.device)
                keep += [values, table]
                job.attr, job.table, job.n = values.data_ptr(), table.data_ptr(), table.shape[0]
                job.lo, job.hi = float(scalar_range[0]), float(scalar_range[1])
            out[name] = torch.empty((self.H, self.W, 3), dtype=torch.uint8, device=self.device)
            job.out = out[name].data_ptr()
        m = np.ascontiguousarray(_host(w2c), dtype=np.float32)
        fx, fy, cx, cy = _pinhole(intrinsics)
        depth, face = self.depth.render(m, intrinsics, near)
        _abi.call(_lib.hsr_mesh_shade, "hsr_mesh_shade", self.device, self.vertices.shape[0], self.faces.shape[0], self.vertices.data_ptr(),
                  self.faces.data_ptr(), self.H, self.W, fx, fy, cx, cy, m.ctypes.data_as(_abi.fp), face.data_ptr(), len(pictures), jobs)
        del keep      # the stream orders the allocator's reuse after the launch
        out["depth"], out["face"] = depth, face
        return out


def vertex_errors(vertices, points, cell=None):
    """float32 [V] on the device: the distance from every vertex to the nearest of points [M,3], exact (mesh_eval.NearestGrid); +inf
    for a vertex with a NaN.  The heat map of the figures: the "scalar" picture of a run's mesh with its errors against samples of the
    ground truth shows accuracy; the ground truth's mesh with its errors against samples of the run's mesh shows completion.  cell:
    the grid's cell, default the box's diagonal over 64 (one host read more than NearestGrid's own)."""
    from .mesh_eval import NearestGrid
    v = _device_tensor(vertices, "vertices", torch.float32, 3)
    pts = _device_tensor(points, "points", torch.float32, 3, v.device)
    if cell is None:
        finite = pts[torch.isfinite(pts).all(dim=1)]
        if finite.shape[0] == 0:
            raise ValueError("hsr_utils.mesh_view: no finite point to measure against")
        cell = max(float((finite.max(dim=0).values - finite.min(dim=0).values).double().norm()) / 64.0, 1e-6)
    d2, _index = NearestGrid(pts, cell).query(v)
    return torch.sqrt(d2)


def orbit_views(lo, hi, n, elevation_deg=30.0, distance=None, up=None):
    """n world-to-camera matrices, float32 [n,4,4] (numpy), on a circle round the box lo..hi, every camera looking at the box's
    centre.  Host arithmetic in float64; the same views from the same arguments.  The construction:
        centre = (lo + hi) / 2;  distance defaults to 1.5 * |hi - lo| (the box's diagonal), and must be positive
        up defaults to (0, -1, 0), minus the image-down axis of a world that is the first camera's frame;  u = up / |up|
        a = the unit vector perpendicular to u from the world axis e with the smallest |e . u| (the lowest index on ties):
            a = (e - (e . u) u) / |..|;   b = u x a
        view i, with phi = 2 pi i / n and theta = elevation_deg in radians:
            eye = centre + distance * (cos(theta) * (cos(phi) * a + sin(phi) * b) + sin(theta) * u)
            f = (centre - eye) / distance, the viewing axis
            |f x u| >= 1e-6:  right = ((-u) x f) / |(-u) x f|  (minus up is the hint for image-down, as virtual_views takes a pose's)
            else (looking straight along u):  right = a
            down = f x right
        the rotation has the rows right, down, f, and the translation is -(that rotation) eye."""
    lo, hi = np.asarray(_host(lo), dtype=np.float64).reshape(3), np.asarray(_host(hi), dtype=np.float64).reshape(3)
    n = int(n)
    if n < 0:
        raise ValueError("hsr_utils.mesh_view: the number of views must be >= 0 (got %d)" % n)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("hsr_utils.mesh_view: the box must be finite (got %s .. %s)" % (lo, hi))
    centre = (lo + hi) / 2
    distance = 1.5 * float(np.linalg.norm(hi - lo)) if distance is None else float(distance)
    if not (np.isfinite(distance) and distance > 0):
        raise ValueError("hsr_utils.mesh_view: distance must be finite and positive (got %r)" % distance)
    u = np.array([0.0, -1.0, 0.0]) if up is None else np.asarray(_host(up), dtype=np.float64).reshape(3)
    if not np.linalg.norm(u) > 0:
        raise ValueError("hsr_utils.mesh_view: up must not be zero")
    u = u / np.linalg.norm(u)
    e = np.eye(3)[int(np.argmin(np.abs(u)))]
    a = e - (e @ u) * u
    a = a / np.linalg.norm(a)
    b = np.cross(u, a)
    theta = np.deg2rad(float(elevation_deg))
    out = np.zeros((n, 4, 4), np.float32)
    for i in range(n):
        phi = 2 * np.pi * i / n
        eye = centre + distance * (np.cos(theta) * (np.cos(phi) * a + np.sin(phi) * b) + np.sin(theta) * u)
        f = (centre - eye) / distance
        if np.linalg.norm(np.cross(f, u)) >= 1e-6:
            right = np.cross(-u, f)
            right = right / np.linalg.norm(right)
        else:
            right = a
        down = np.cross(f, right)
        view = np.eye(4)
        view[:3, :3] = np.stack([right, down, f])
        view[:3, 3] = -view[:3, :3] @ eye
        out[i] = view
    return out


def _mesh_parts(mesh):
    """(vertices, faces, rgb, labels) of a two- to four-tuple"""
    parts = tuple(mesh) + (None,) * (4 - len(mesh))
    if len(parts) != 4:
        raise RuntimeError("hsr_utils.mesh_view: a mesh is (vertices, faces[, rgb[, labels]])")
    return parts


def render_mesh_views(mesh, w2cs, intrinsics, H, W, out_dir=None, pictures=("shaded",), gt=None, normals="smooth", scalar=None,
                      scalar_range=None, error_samples=200000, seed=0, **render_kw):
    """The pictures of mesh = (vertices, faces[, rgb[, labels]]) from every view of w2cs [T,4,4].  Without out_dir: a list of T
    dicts, MeshRenderer.render's.  With out_dir: the files {picture}_{i:04d}.png (export.write_png) and the list of their paths.
    gt = (vertices, faces) of the ground truth in the same frame: its "shaded" picture from the same views as gt_shaded_{i:04d}.png
    (key "gt_shaded" of the dicts), and, when "scalar" is asked without a scalar, scalar = vertex_errors(vertices, sample_mesh(gt,
    error_samples, seed)) — the accuracy heat map — with scalar_range defaulting to (0, the 95th percentile of the finite errors): one
    host read, once.  render_kw goes to MeshRenderer.render (near, ambient, albedo, background, the tables, lit)."""
    vertices, faces, rgb, labels = _mesh_parts(mesh)
    views = _views(w2cs)
    pictures = (pictures,) if isinstance(pictures, str) else tuple(pictures)
    renderer = MeshRenderer(vertices, faces, H, W, rgb=rgb, labels=labels, normals=normals)
    dev = renderer.device
    gt_renderer = None
    if gt is not None:
        gt_renderer = MeshRenderer(_device_tensor(gt[0], "gt vertices", torch.float32, 3, dev),
                                   _device_tensor(gt[1], "gt faces", torch.int32, 3, dev), H, W, normals=normals)
    if "scalar" in pictures:
        if scalar is None:
            if gt_renderer is None:
                raise RuntimeError("hsr_utils.mesh_view: the \"scalar\" picture needs scalar= or gt= to measure the errors against")
            from .mesh_eval import sample_mesh
            points = sample_mesh(gt_renderer.vertices, gt_renderer.faces, int(error_samples), seed)[0]
            scalar = vertex_errors(renderer.vertices, points)
        if scalar_range is None:
            values = _device_tensor(scalar, "scalar", torch.float32, None, dev)
            finite = values[torch.isfinite(values)]
            top = float(torch.quantile(finite.double(), 0.95)) if finite.numel() else 0.0      # the one host read
            scalar_range = (0.0, top if top > 0 else 1.0)
    shade_kw = {k: render_kw[k] for k in ("near", "ambient", "albedo", "background") if k in render_kw}
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        from .export import write_png
    results = []
    for i, m in enumerate(views):
        got = renderer.render(m, intrinsics, pictures, scalar=scalar, scalar_range=scalar_range, **render_kw)
        if gt_renderer is not None:
            got["gt_shaded"] = gt_renderer.render(m, intrinsics, ("shaded",), **shade_kw)["shaded"]
        if out_dir is None:
            results.append(got)
            continue
        for name in pictures + (("gt_shaded",) if gt_renderer is not None else ()):
            path = os.path.join(out_dir, "%s_%04d.png" % (name, i))
            write_png(path, got[name])
            results.append(path)
    return results


def render_mesh_run(params, mesh, out_dir, every=50, orbit=0, intrinsics=None, width=None, height=None, num_frames=None, first_frame_w2c=None,
                    size=None, elevation_deg=30.0, **kw):
    """The pictures of a finished run's mesh, mesh = (vertices, faces[, rgb[, labels]]) as load_mesh_ply returns it, into out_dir:
    from every `every`-th estimated pose of the run — replay.run_w2cs(params), each after first_frame_w2c (default params['w2c'],
    else the identity), exactly the views mesh_run fuses from — and from `orbit` orbit_views round the mesh's bounds.  intrinsics,
    width, height and num_frames default to the params' 'intrinsics', 'org_width', 'org_height' and the number of pose columns;
    size = (W, H) renders at another size with the intrinsics scaled per axis.  kw goes to render_mesh_views (pictures, gt, normals,
    the scalar and the shading keywords).  Returns the list of paths; the file index counts the pose views first, then the orbit."""
    from .replay import run_w2cs
    if int(every) < 1:
        raise ValueError("hsr_utils.mesh_view: every must be >= 1")
    dev = params['means3D'].device      # arrays, as load_mesh_ply returns them, go where the run's map is
    mesh = tuple(None if part is None else (part if isinstance(part, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(part), device=dev))
                 for part in _mesh_parts(mesh))
    k = np.array(np.asarray(_host(params['intrinsics'] if intrinsics is None else intrinsics), dtype=np.float64)[:3, :3])
    w = int(_host(params['org_width'])) if width is None else int(width)
    h = int(_host(params['org_height'])) if height is None else int(height)
    T = int(params['cam_unnorm_rots'].shape[-1]) if num_frames is None else int(num_frames)
    if first_frame_w2c is None:
        first_frame_w2c = params['w2c'] if 'w2c' in params else np.eye(4)
    first = np.asarray(_host(first_frame_w2c), dtype=np.float32)
    if first.shape != (4, 4):
        raise RuntimeError("hsr_utils.mesh_view: first_frame_w2c must be [4,4] (got %s)" % (first.shape,))
    if size is not None:
        k[0] *= float(size[0]) / w
        k[1] *= float(size[1]) / h
        w, h = int(size[0]), int(size[1])
    views = run_w2cs(params).cpu().numpy()[:T]      # one copy for the run
    if not np.array_equal(first, np.eye(4, dtype=np.float32)):
        views = np.stack([first @ m for m in views]) if len(views) else views
    views = np.asarray(views, dtype=np.float32)[::int(every)]
    if int(orbit) > 0:
        vertices = _mesh_parts(mesh)[0]
        v = vertices if isinstance(vertices, torch.Tensor) else torch.as_tensor(np.asarray(vertices))
        v = v[torch.isfinite(v).all(dim=1)]
        if v.shape[0] == 0:
            raise ValueError("hsr_utils.mesh_view: the mesh has no finite vertex to orbit")
        views = np.concatenate([views.reshape(-1, 4, 4), orbit_views(v.min(dim=0).values.cpu().numpy(), v.max(dim=0).values.cpu().numpy(),
                                                                     int(orbit), elevation_deg=elevation_deg)])
    return render_mesh_views(mesh, views, k, h, w, out_dir=out_dir, **kw)


__all__ = ["vertex_normals", "MeshRenderer", "vertex_errors", "orbit_views", "render_mesh_views", "render_mesh_run"]
