"""A numpy restatement of include/surface/hsr_mesh_clean.h, rule by rule: what hsr_mesh_components and hsr_mesh_select must produce, and
hsr_utils.mesh_clean.component_keep's rule once more.  Integers only, so the device is expected to give these arrays EXACTLY.  Written
from the header alone: the C code is not read.  The components come from a sequential union-find that links the larger root under the
smaller one; flood_fill is the same relation by brute force, for the tests of this file's own correctness."""
import math

import numpy as np

BLOCK = 256      # HSR_MESH_CLEAN_BLOCK


def valid_faces(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(axis=1)


def components(faces, V, order=None):
    """(label int32 [V], face_count int32 [V]).  `order`: the order in which the faces are united (default: as they come); the result
    must not depend on it."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_faces(f, V)
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i in (range(len(f)) if order is None else order):
        if not ok[i]:
            continue
        a, b, c = (int(t) for t in f[i])
        for p, q in ((a, b), (b, c)):
            rp, rq = find(p), find(q)
            if rp != rq:
                parent[max(rp, rq)] = min(rp, rq)
    label = np.array([find(v) for v in range(V)], np.int32).reshape(V)
    count = np.zeros(V, np.int32)
    if ok.any():
        np.add.at(count, label[f[ok, 0]], 1)
    return label, count


def flood_fill(faces, V):
    """the same two arrays by brute force: adjacency sets and a search from every vertex not yet reached, in ascending order"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_faces(f, V)
    near = [set() for _ in range(V)]
    for a, b, c in f[ok]:
        for p, q in ((a, b), (b, c), (c, a)):
            near[p].add(int(q))
            near[q].add(int(p))
    label = np.full(V, -1, np.int32)
    for start in range(V):
        if label[start] >= 0:
            continue
        label[start] = start      # the smallest index of its component: everything below it is labelled already
        stack = [start]
        while stack:
            for q in near[stack.pop()]:
                if label[q] < 0:
                    label[q] = start
                    stack.append(q)
    count = np.zeros(V, np.int32)
    for a in f[ok, 0]:
        count[label[a]] += 1
    return label, count


def keep(face_count, min_faces=0, min_ratio=0.0, largest=False):
    """component_keep's rule: uint8 [V]"""
    count = np.asarray(face_count, np.int64)
    if count.size == 0:
        return np.zeros(0, np.uint8)
    top = int(count.max())
    thr = max(int(min_faces), int(math.ceil(float(top) * float(min_ratio))), 1)
    out = count >= thr
    if largest:
        first = np.zeros_like(out)
        first[int(np.argmax(count == top))] = True
        out &= first
    return out.astype(np.uint8)


def select(faces, V, label, keep_by_label):
    """(out_faces int32 [F',3], out_source int32 [V']): the written parts of the header's outputs; the counts are their lengths"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    label, keep_by_label = np.asarray(label, np.int64), np.asarray(keep_by_label)
    kept = valid_faces(f, V)
    if kept.any():
        r = label[f[kept, 0]]
        inside = (r >= 0) & (r < V)
        good = np.zeros(len(r), bool)
        good[inside] = keep_by_label[r[inside]] != 0
        kept[np.flatnonzero(kept)] = good
    used = np.zeros(V, bool)
    used[f[kept].reshape(-1)] = True
    source = np.flatnonzero(used).astype(np.int32)
    new_index = np.cumsum(used) - 1
    return new_index[f[kept]].astype(np.int32).reshape(-1, 3), source


def clean(vertices, faces, min_faces=0, min_ratio=0.0, largest=False):
    """clean_mesh on arrays: (vertices, faces, source)"""
    V = len(vertices)
    label, count = components(faces, V)
    out_faces, source = select(faces, V, label, keep(count, min_faces, min_ratio, largest))
    return np.asarray(vertices)[source], out_faces, source


# ---- the meshes of the tests ----------------------------------------------------------------------------------------------------------------
def strip(n, numbering="ascending", seed=0):
    """a triangle strip of n faces over n + 2 vertices, face i = (i, i + 1, i + 2) before the renumbering"""
    i = np.arange(n, dtype=np.int64)
    f = np.stack([i, i + 1, i + 2], axis=1)
    V = n + 2
    if numbering == "descending":
        f = V - 1 - f
    elif numbering == "permuted":
        f = np.random.default_rng(seed).permutation(V)[f]
    else:
        assert numbering == "ascending"
    return f.astype(np.int32), V


def fan(n, hub="first"):
    """n faces around one vertex: (hub, rim i, rim i + 1) over n + 2 vertices; hub = "first": vertex 0, "last": the largest index"""
    i = np.arange(n, dtype=np.int64)
    V = n + 2
    if hub == "first":
        f = np.stack([np.zeros(n, np.int64), i + 1, i + 2], axis=1)
    else:
        f = np.stack([np.full(n, V - 1, np.int64), i, i + 1], axis=1)
    return f.astype(np.int32), V


def disjoint(n):
    """n faces that share nothing, over 3 n vertices"""
    return np.arange(3 * n, dtype=np.int32).reshape(n, 3), 3 * n


def patches(side=70, cuts=(9, 10, 20, 21, 24, 25, 37, 38, 50, 51), seed=0):
    """a side x side grid of vertices, two faces a cell, cut into rectangular patches by leaving out the cells of the rows and columns
    in `cuts` (the vertices stay: those between two neighbouring cuts are named by no face); vertex numbers randomly permuted, face order shuffled.
    Returns (faces int32 [F,3], V, number of patches)."""
    rng = np.random.default_rng(seed)
    cells = [(r, c) for r in range(side - 1) for c in range(side - 1) if r not in cuts and c not in cuts]
    r, c = np.array(cells, np.int64).T
    v00, v01, v10, v11 = r * side + c, r * side + c + 1, (r + 1) * side + c, (r + 1) * side + c + 1
    f = np.concatenate([np.stack([v00, v01, v11], axis=1), np.stack([v00, v11, v10], axis=1)])
    V = side * side
    f = rng.permutation(V)[f]
    f = f[rng.permutation(len(f))]

    def bands(n):
        out, run = 0, False
        for i in range(n):
            inside = i not in cuts
            out += inside and not run
            run = inside
        return out

    return f.astype(np.int32), V, bands(side - 1) ** 2
