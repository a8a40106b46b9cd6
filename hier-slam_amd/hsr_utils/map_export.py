"""The finished map as the point clouds people look at, on the device (include/ext/hsr_map_export.h): what the
reference's scripts/export_ply_semantic_tree.py does between the arrays of params.npz and PlyData.write — save_ply (:251-277),
save_ply_semantic (:279-327) with transfer_tree_label (:208-228) and semantic_label_vis (:230-248), save_ply_semantic_multilevel
(:329-382) with transfer_eachlevel_1 (:183-199), and the leaf-head colouring (flag_mlp_show = 1, :286-294).

    gaussian_tree_labels(semantic, level_sizes)                     int32 [L,P] on the device: transfer_tree_label
    export_map(params, colour=..., ...)                             ONE launch: (body, fields), the PLY body as a uint8 device tensor
    level_prefix_colour_table(tree_id_classes_map_level, level_sizes, i_level, device)
                                                                    the colour table of save_ply_semantic_multilevel, uint8 [prod,3]
    leaf_head_labels(semantic, mlp)                                 int32 [P]: the class ids of the leaf head (evaluate.semantic_labels)
    ply_header(count, fields)                                       the header map_io.write_ply writes, as bytes
    save_map_ply(path, params, **kw)                                header, one device-to-host copy of the body, one write
    save_map_ply_semantic(path, params, colour_map_level, level_sizes, wildcard=..., ...)

The files equal those of the host writers hsr_utils.map_io.save_ply / save_ply_semantic byte for byte.  There is no CPU path; map_io
stays the host-side writer.  The colour tables are built on the host with numpy, once (hsr_utils.export).
"""
import numpy as np
import torch

from diff_gaussian_rasterization import _abi
from . import export
from .evaluate import _dev, tree_levels

_lib = _abi.lib

MAP_EXPORT_MAX_P = 31580641                      # HSR_MAP_EXPORT_MAX_P
RECORD_SH, RECORD_RGB8, RECORD_NONE = 0, 1, 2    # HSR_MAP_RECORD_*
COLOUR_GIVEN, COLOUR_LABELS, COLOUR_TREE = 0, 1, 2      # HSR_MAP_COLOUR_*
RECORD_BYTES = {RECORD_SH: 68, RECORD_RGB8: 59}
COLOURS = ("sh", "given", "labels", "tree")

_GEOMETRY = tuple(("float", n) for n in ("x", "y", "z", "nx", "ny", "nz"))
_REST = tuple(("float", n) for n in ("opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"))
FIELDS_SH = _GEOMETRY + tuple(("float", n) for n in ("f_dc_0", "f_dc_1", "f_dc_2")) + _REST
FIELDS_RGB8 = _GEOMETRY + tuple(("uchar", n) for n in ("red", "green", "blue")) + _REST


def _array(t, what, cols, P=None, dtype=torch.float32):
    """a [P,cols] array of the map ([P] also for cols = 1) as a contiguous device tensor: detached views and non-contiguous tensors are
    made contiguous, nothing else is copied"""
    if isinstance(t, torch.Tensor):
        t = t.detach()
    t = _dev(t, what, dtype)
    ok = (t.dim() == 2 and t.shape[1] in cols) or (1 in cols and t.dim() == 1)
    if not ok or (P is not None and t.shape[0] != P):
        raise RuntimeError("hsr_utils.map_export: %s must be [%s,%s] (got %s)"
                           % (what, "P" if P is None else P, "|".join(str(c) for c in cols), tuple(t.shape)))
    return t


def _tree_job(job, semantic, level_sizes, P=None):
    sizes, n = tree_levels(level_sizes)
    sem = _dev(semantic.detach() if isinstance(semantic, torch.Tensor) else semantic, "semantic")
    if sem.dim() != 2 or sem.shape[1] < sum(sizes) or (P is not None and sem.shape[0] != P):
        raise RuntimeError("hsr_utils.map_export: semantic must be [%s,K] with K >= %d, the levels %s (got %s)"
                           % ("P" if P is None else P, sum(sizes), sizes, tuple(sem.shape)))
    job.semantic, job.K, job.L = sem.data_ptr(), int(sem.shape[1]), len(sizes)
    job.sizes[:len(sizes)] = sizes
    return sem, sizes, n


def _count(P):
    if P > MAP_EXPORT_MAX_P:
        raise ValueError("hsr_utils.map_export: a map of %d Gaussians; one call takes %d at the most" % (P, MAP_EXPORT_MAX_P))
    return P


def gaussian_tree_labels(semantic, level_sizes):
    """int32 [L,P] on the device: per Gaussian and level the argmax(softmax(.)) of the level's columns of semantic ([P,K] float32), the
    device form of transfer_tree_label (scripts/export_ply_semantic_tree.py:208-228).  level_sizes is the dataset's num_semantic, whose
    last entry, the leaf count, is dropped.  The labels are those of evaluate.semantic_labels(mode="tree") on the same logits, bit for
    bit: ties are among the fp32 probabilities and go to the lowest index."""
    job = _abi.hsr_map_export_job(record=RECORD_NONE)
    sem, sizes, _n = _tree_job(job, semantic, level_sizes)
    P = _count(int(sem.shape[0]))
    out = torch.empty((len(sizes), P), dtype=torch.int32, device=sem.device)
    job.P, job.out_labels = P, out.data_ptr()
    _abi.call(_lib.hsr_map_export, "hsr_map_export", sem.device, job)
    return out


def export_map(params, *, colour="sh", colours=None, labels=None, table=None, level_sizes=None, normals=None, return_labels=False):
    """The body of the map's PLY file from ONE hsr_map_export launch: (body, fields), body a uint8 device tensor of P records and fields
    the header's property list, ((type, name), ...).  params is the map dict: means3D [P,3], rgb_colors [P,3], unnorm_rotations [P,4],
    logit_opacities [P,1], log_scales [P,1|3] (one log-scale goes out three times) and, for colour="tree", semantic [P,K]; the rest of
    the dict is ignored.  normals [P,3] or None for zeros.
      colour "sh"      68-byte records, the colour as f_dc_c = (rgb_c - 0.5) / C0 in fp32 (save_ply, :251-277);
      colour "given"   59-byte records with colours uint8 [P,3] as red green blue (save_ply_semantic after its lookup, :300-327);
      colour "labels"  ... with table[label] for labels int32 [P] and table uint8 [n,3]; black outside the table (:294, :352);
      colour "tree"    ... with table[tuple of the per-level labels], table uint8 [prod(sizes),3] (export.tuple_colour_table or
                       level_prefix_colour_table) and level_sizes the dataset's num_semantic, whose last entry is dropped (:296-298).
                       return_labels=True also returns those labels, int32 [L,P]: (body, fields, labels).
    Logits, log-scales and quaternions go out as stored; every float but f_dc_* is a bit copy.  Detached views and non-contiguous tensors
    are made contiguous; nothing else is copied and nothing synchronises.  There is no CPU path."""
    if colour not in COLOURS:
        raise ValueError("hsr_utils.map_export: colour must be one of %s (got %r)" % (", ".join(COLOURS), colour))
    if return_labels and colour != "tree":
        raise ValueError("hsr_utils.map_export: return_labels goes with colour='tree'")
    means = _array(params["means3D"], "means3D", (3,))
    P, dev = _count(int(means.shape[0])), means.device
    rot = _array(params["unnorm_rotations"], "unnorm_rotations", (4,), P)
    opac = _array(params["logit_opacities"], "logit_opacities", (1,), P)
    scales = _array(params["log_scales"], "log_scales", (1, 3), P)
    keep = [means, rot, opac, scales]
    job = _abi.hsr_map_export_job(P=P, S=1 if scales.dim() == 1 else int(scales.shape[1]), means3D=means.data_ptr(),
                                  unnorm_rotations=rot.data_ptr(), logit_opacities=opac.data_ptr(), log_scales=scales.data_ptr())
    if normals is not None:
        normals = _array(normals, "normals", (3,), P)
        job.normals = normals.data_ptr()
        keep.append(normals)
    out_labels = None
    if colour == "sh":
        rgb = _array(params["rgb_colors"], "rgb_colors", (3,), P)
        job.record, job.rgb_colors = RECORD_SH, rgb.data_ptr()
        keep.append(rgb)
    else:
        job.record = RECORD_RGB8
        if colour == "given":
            if colours is None:
                raise RuntimeError("hsr_utils.map_export: colour='given' needs colours")
            colours = _array(colours, "colours", (3,), P, torch.uint8)
            job.colour, job.colours = COLOUR_GIVEN, colours.data_ptr()
            keep.append(colours)
        else:
            if table is None or (labels is None if colour == "labels" else level_sizes is None):
                raise RuntimeError("hsr_utils.map_export: colour='labels' needs labels and table, colour='tree' level_sizes and table")
            if colour == "labels":
                labels = _array(labels, "labels", (1,), P, torch.int32)
                table = export._table(table, "table")
                job.colour, job.labels = COLOUR_LABELS, labels.data_ptr()
                keep.append(labels)
            else:
                sem, sizes, n = _tree_job(job, params["semantic"], level_sizes, P)
                table = export._table(table, "table", n)
                job.colour = COLOUR_TREE
                keep.append(sem)
                if return_labels:
                    out_labels = torch.empty((len(sizes), P), dtype=torch.int32, device=dev)
                    job.out_labels = out_labels.data_ptr()
            job.table, job.n = table.data_ptr(), int(table.shape[0])
            keep.append(table)
    for t in keep:
        if t.device != dev:
            raise RuntimeError("hsr_utils.map_export: the map is on %s, one of its arrays or tables on %s" % (dev, t.device))
    body = torch.empty(P * RECORD_BYTES[job.record], dtype=torch.uint8, device=dev)
    job.out = body.data_ptr()
    _abi.call(_lib.hsr_map_export, "hsr_map_export", dev, job)
    fields = FIELDS_SH if colour == "sh" else FIELDS_RGB8
    return (body, fields, out_labels) if return_labels else (body, fields)


def level_prefix_colour_table(tree_id_classes_map_level, level_sizes, i_level, device="cuda"):
    """The colours of save_ply_semantic_multilevel (scripts/export_ply_semantic_tree.py:347-352) for level i_level as a dense
    uint8 [prod(level_sizes[:i_level + 1]), 3] table over the mixed-radix index of the first i_level + 1 level labels:
    tree_id_classes_map_level is the dataset's tree_id_classes_map[i_level], a dict whose keys are the label tuples of those levels; a
    tuple takes the colour label_colormap(len(dict))[position of its key in the dict] (transfer_eachlevel_1, :183-199).  Of two equal
    keys the later one wins, as the reference's loop of masked assignments does.  A tuple no key names is BLACK here: the reference
    leaves it at -1, which numpy wraps to the LAST colour of the map — deliberately not copied.  level_sizes is the dataset's
    num_semantic (the leaf count last).  Exporting level i is then colour="tree" with this table and the first i + 1 level sizes (plus
    any last entry, which is dropped): save_map_ply_semantic(i_level=...) does both."""
    sizes, _n = tree_levels(level_sizes)
    i_level = int(i_level)
    if not 0 <= i_level < len(sizes):
        raise ValueError("hsr_utils.map_export: i_level must be 0..%d (got %d)" % (len(sizes) - 1, i_level))
    cmap = export.label_colormap(len(tree_id_classes_map_level), "cpu").tolist()
    colour_map = {key: cmap[position] for position, key in enumerate(tree_id_classes_map_level)}
    return export.tuple_colour_table(colour_map, sizes[:i_level + 1] + [0], False, device=device)


def leaf_head_labels(semantic, mlp):
    """int32 [P]: the class ids of the leaf head on the map's logits (flag_mlp_show = 1, :286-294): evaluate.semantic_labels(mode="leaf")
    on semantic [P,K] viewed as a [K,1,P] image.  A composition, no new arithmetic; colour="labels" then looks the ids up."""
    from . import evaluate
    sem = _dev(semantic.detach() if isinstance(semantic, torch.Tensor) else semantic, "semantic")
    if sem.dim() != 2:
        raise RuntimeError("hsr_utils.map_export: semantic must be [P,K] (got %s)" % (tuple(sem.shape),))
    return evaluate.semantic_labels(sem.t().contiguous().view(sem.shape[1], 1, sem.shape[0]), "leaf", mlp=mlp).view(-1)


def ply_header(count, fields):
    """the header hsr_utils.map_io.write_ply writes for one `vertex` element of `count` records with the properties `fields`"""
    lines = ["ply", "format binary_little_endian 1.0", "element vertex %d" % count] + ["property %s %s" % f for f in fields] + ["end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def _write(path, body, fields):
    record = sum(4 if kind == "float" else 1 for kind, _name in fields)
    host = body.cpu().numpy()      # the one device-to-host copy
    with open(path, "wb") as f:
        f.write(ply_header(host.size // record, fields))
        f.write(memoryview(host))
    return path


def save_map_ply(path, params, **kw):
    """export_map(params, **kw) as a PLY file: the header of map_io.write_ply, one device-to-host copy of the body, one write.  With the
    default colour="sh" the file is map_io.save_ply's, byte for byte."""
    if kw.get("return_labels"):
        raise ValueError("hsr_utils.map_export: save_map_ply writes a file; use export_map for the labels")
    body, fields = export_map(params, **kw)
    return _write(path, body, fields)


def save_map_ply_semantic(path, params, colour_map_level, level_sizes, *, wildcard, i_level=None, tree_id_classes_map_level=None,
                          labels=None, table=None):
    """The semantic point cloud of the map, map_io.save_ply_semantic's file byte for byte, coloured
      per tree tuple (save_ply_semantic, :296-298): colour_map_level is the dataset's colour_map_np_level and level_sizes its
          num_semantic; wildcard as in export.tuple_colour_table (True: Replica's -1 keys match every label);
      per level (save_ply_semantic_multilevel, :347-352) with i_level and tree_id_classes_map_level = the dataset's
          tree_id_classes_map[i_level]: the first i_level + 1 levels, coloured by level_prefix_colour_table;
      per class (flag_mlp_show = 1, :286-294) with labels (leaf_head_labels) and table (export.label_colormap, or the dataset's
          colors_map_all): colour_map_level and level_sizes are then not read."""
    dev = params["means3D"].device
    if labels is not None or table is not None:
        if labels is None or table is None or i_level is not None:
            raise RuntimeError("hsr_utils.map_export: labels and table go together, without i_level")
        body, fields = export_map(params, colour="labels", labels=labels, table=table)
    elif i_level is not None:
        if tree_id_classes_map_level is None:
            raise RuntimeError("hsr_utils.map_export: i_level needs tree_id_classes_map_level")
        sizes = [int(s) for s in level_sizes]
        prefix = level_prefix_colour_table(tree_id_classes_map_level, sizes, i_level, dev)
        body, fields = export_map(params, colour="tree", table=prefix, level_sizes=sizes[:int(i_level) + 1] + sizes[-1:])
    else:
        tuples = export.tuple_colour_table(colour_map_level, level_sizes, wildcard, dev)
        body, fields = export_map(params, colour="tree", table=tuples, level_sizes=level_sizes)
    return _write(path, body, fields)


__all__ = ["gaussian_tree_labels", "export_map", "level_prefix_colour_table", "leaf_head_labels", "ply_header", "save_map_ply",
           "save_map_ply_semantic", "FIELDS_SH", "FIELDS_RGB8"]
