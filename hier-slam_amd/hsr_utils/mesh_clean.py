"""Small connected components off a mesh, on the device (include/surface/hsr_mesh_clean.h): the step between
TsdfVolume.extract and the scores of mesh_eval / mesh_depth.  Floaters, silhouette fringes and stray blobs behind thin structures come
out of the volume as little shells, and every surface sample drawn on them counts against accuracy, F-score and Depth L1.  What the
reference family does with Open3D (cluster_connected_triangles, remove_triangles_by_mask, remove_unreferenced_vertices); the reference
itself has no mesh, so the rules are this project's own and the header states each of them.

    mesh_components(faces, num_vertices)    (label int32 [V], face_count int32 [V]) on the device: ONE hsr_mesh_components, no host read
    component_keep(face_count, min_faces=0, min_ratio=0.0, largest=False)    uint8 [V], plain torch on the tensor's device, no host read
    clean_mesh(vertices, faces, rgb=None, labels=None, *, min_faces=0, min_ratio=0.0, largest=False)
        mesh_components, component_keep, ONE hsr_mesh_select, ONE host read (three words), one index_select per attribute

mesh.mesh_run takes min_component_faces, min_component_ratio and largest_component and cleans between extract and save_mesh_ply;
mesh_eval.evaluate_mesh_run, SlamSession.export_mesh and SlamSession.evaluate_mesh forward their keywords to it.  There is no CPU path
for anything that launches; component_keep runs anywhere.
"""
import math

import torch

from diff_gaussian_rasterization import _abi

_lib = _abi.lib

BLOCK = 256      # HSR_MESH_CLEAN_BLOCK: the items of one block of the compaction


def _faces(faces, num_vertices):
    V = int(num_vertices)
    if V < 0 or V > 2 ** 31 - 1:
        raise ValueError("hsr_utils.mesh_clean: the number of vertices must be 0..2^31-1 (got %d)" % V)
    if not isinstance(faces, torch.Tensor) or not faces.is_cuda:
        raise RuntimeError("hsr_utils.mesh_clean: faces must be a tensor on a HIP device; there is no CPU path")
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("hsr_utils.mesh_clean: faces must be int32 [F,3] (got %s %s)" % (faces.dtype, tuple(faces.shape)))
    return faces.detach().contiguous(), V


def mesh_components(faces, num_vertices):
    """(label int32 [V], face_count int32 [V]) of the mesh of `faces` (int32 [F,3], on the device) over num_vertices vertices: label[v]
    is the smallest vertex index of v's component, face_count[r] the number of valid faces of the component whose label is r and 0
    elsewhere.  A face with an index outside 0..V-1 connects nothing and is counted nowhere.  ONE call, no host read; a negative
    face_count says that a walk gave up (the header's rule; clean_mesh checks it)."""
    faces, V = _faces(faces, num_vertices)
    dev = faces.device
    label = torch.empty(V, dtype=torch.int32, device=dev)
    count = torch.empty(V, dtype=torch.int32, device=dev)
    F = int(faces.shape[0])
    _abi.call(_lib.hsr_mesh_components, "hsr_mesh_components", dev, V, F, faces.data_ptr() if F else None, label.data_ptr() if V else None,
              count.data_ptr() if V else None)
    return label, count


def component_keep(face_count, min_faces=0, min_ratio=0.0, largest=False):
    """uint8 [V], 1 at the labels of the components to keep, from face_count of mesh_components.  thr = max(min_faces,
    ceil(float64(largest count) * float64(min_ratio))) and keep = face_count >= max(thr, 1): an index that is no label has a count of 0
    and is never kept.  largest=True keeps ONLY the first index that holds the largest count, a tie going to the smallest label (and
    nothing when there is no face at all); min_faces and min_ratio still apply to it.  Plain torch on face_count's device, no host read."""
    min_faces, min_ratio = int(min_faces), float(min_ratio)
    if min_faces < 0:
        raise ValueError("hsr_utils.mesh_clean: min_faces must be >= 0 (got %d)" % min_faces)
    if not (math.isfinite(min_ratio) and 0.0 <= min_ratio <= 1.0):
        raise ValueError("hsr_utils.mesh_clean: min_ratio must be in [0, 1] (got %r)" % min_ratio)
    count = face_count.detach().to(torch.int64)
    if count.numel() == 0:
        return torch.zeros(0, dtype=torch.uint8, device=count.device)
    top = count.max()
    by_ratio = torch.ceil(top.to(torch.float64) * min_ratio).to(torch.int64)
    thr = torch.clamp_min(torch.clamp_min(by_ratio, min_faces), 1)
    keep = count >= thr
    if largest:
        first = torch.zeros_like(keep)
        first[torch.argmax((count == top).to(torch.uint8))] = True      # argmax of a 0/1 tensor: the first 1
        keep = keep & first
    return keep.to(torch.uint8)


def clean_mesh(vertices, faces, rgb=None, labels=None, *, min_faces=0, min_ratio=0.0, largest=False):
    """(vertices float32 [V',3], faces int32 [F',3], rgb uint8 [V',3] | None, labels int32 [V'] | None) without the components that
    component_keep(min_faces, min_ratio, largest) does not keep and without the vertices no kept face names; kept faces and kept
    vertices keep their order.  Takes what TsdfVolume.extract returns.  ONE host read, of {F', V', gave_up}: it sizes the outputs, and
    a gave_up that is not 0 raises RuntimeError (the header's rule: it cannot happen).  An empty mesh gives empty tensors."""
    if not isinstance(vertices, torch.Tensor) or not vertices.is_cuda:
        raise RuntimeError("hsr_utils.mesh_clean: vertices must be a tensor on a HIP device; there is no CPU path")
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise RuntimeError("hsr_utils.mesh_clean: vertices must be [V,3] (got %s)" % (tuple(vertices.shape),))
    faces, V = _faces(faces, vertices.shape[0])
    dev = vertices.device
    if faces.device != dev:
        raise RuntimeError("hsr_utils.mesh_clean: faces are on %s, vertices on %s" % (faces.device, dev))
    for name, t, shape in (("rgb", rgb, (V, 3)), ("labels", labels, (V,))):
        if t is not None and (not isinstance(t, torch.Tensor) or t.device != dev or tuple(t.shape) != shape):
            raise RuntimeError("hsr_utils.mesh_clean: %s must be a tensor %s on %s" % (name, list(shape), dev))
    F = int(faces.shape[0])
    label, count = mesh_components(faces, V)
    keep = component_keep(count, min_faces, min_ratio, largest)
    out_faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
    source = torch.empty(V, dtype=torch.int32, device=dev)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    need = int(_lib.hsr_mesh_select_scratch_bytes(V, F))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    _abi.call(_lib.hsr_mesh_select, "hsr_mesh_select", dev, V, F, faces.data_ptr() if F else None, label.data_ptr() if V else None,
              keep.data_ptr() if V else None, out_faces.data_ptr() if F else None, source.data_ptr() if V else None, counts.data_ptr(),
              scratch.data_ptr(), need)
    counts[2] += (count < 0).sum()      # the gave_up word of the header, carried by the one read
    nf, nv, gave_up = (int(c) for c in counts.tolist())      # the one host read
    if gave_up != 0:
        raise RuntimeError("hsr_utils.mesh_clean: %d walks of hsr_mesh_components gave up; labels and counts are not to be used" % gave_up)
    src = source[:nv].long()
    return (vertices.index_select(0, src), out_faces[:nf], None if rgb is None else rgb.index_select(0, src),
            None if labels is None else labels.index_select(0, src))


__all__ = ["mesh_components", "component_keep", "clean_mesh"]
