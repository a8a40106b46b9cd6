"""A numpy restatement of include/ext/hsr_frame_ingest_planes.h: what hsr_frame_ingest_planes must produce bit for bit.  The three rules
are those of tests/ingest_ref.py (imported as it is), each applied to its own source array; the leaf-column rule is added here.

    color(color_u8, (h, w)), depth(depth_raw, (h, w), scale)       ingest_ref's, from the image's own size
    labels(ids, (h, w), table | None, leaf_column)                 int64 [L+1,h,w]; table is [n_ids, L + leaf_column]
    frame(color_u8, depth_raw, sizes, scale, ids, table, leaf)     ([(color, depth) per size], labels at sizes[0] | None)
    reference_loops(raw, class_mapping, tree, L)                   the reference's two loops of masked assignments, literally
"""
import numpy as np

import ingest_ref as I

color, depth = I.color, I.depth


def labels(ids, size, table=None, leaf_column=False):
    if not leaf_column:
        return I.labels(ids, size, table)
    table = np.asarray(table, dtype=np.int64)
    L = table.shape[1] - 1
    planes = I.labels(ids, size, table[:, :L] if L else None)      # the level planes, then the raw id
    raw = planes[L]
    known = (raw >= 0) & (raw < table.shape[0])
    planes[L] = np.where(known, table[np.where(known, raw, 0), L], raw)
    return planes


def frame(color_u8, depth_raw, sizes, scale, ids=None, table=None, leaf_column=False):
    levels = [(color(color_u8, hw), depth(depth_raw, hw, scale)) for hw in sizes]
    return levels, (None if ids is None else labels(ids, sizes[0], table, leaf_column))


def reference_loops(raw, class_mapping, tree, L):
    """datasets/gradslam_datasets/scannet.py:288-290, then :302-307 / :325-330 and the stack of :309-314 / :332-338, on an int64 id
    image: every mask is taken from an unchanged array (raw in the first loop, nyu in the second)."""
    raw = np.asarray(raw, dtype=np.int64)
    nyu = raw.copy()
    for scan_id, nyu_id in (class_mapping or {}).items():
        nyu[raw == scan_id] = nyu_id
    levels = [nyu.copy() for _ in range(L)]
    for scan_id, tree_id in (tree or {}).items():
        for l in range(L):
            levels[l][nyu == scan_id] = tree_id[l]
    return np.stack(levels + [nyu])
