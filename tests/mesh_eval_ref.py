"""The numpy restatement of include/eval/hsr_mesh_eval.h for the tests: every float32 operation rounded once, in the header's order, so
that the device's outputs can be compared bit for bit.  Also the grid search of hsr_nn_query as a plain loop (grid_nn), which the CPU
suite holds against brute force (brute_nn): that comparison is the proof of the stopping rule.  And the fixtures both suites share."""
import numpy as np

F32 = np.float32
MASK = (1 << 64) - 1


# ---- areas and samples ------------------------------------------------------------------------------------------------------------------
def areas(vertices, faces):
    v, f = np.asarray(vertices, F32), np.asarray(faces, np.int64)
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    g = np.where(ok[:, None], f, 0)
    A, B, C = v[g[:, 0]], v[g[:, 1]], v[g[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = B - A, C - A
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        area = F32(0.5) * np.sqrt((cx * cx + cy * cy) + cz * cz)
    return np.where(ok & np.isfinite(area), area, F32(0)).astype(F32)


def splitmix(seed, n):
    z = (int(seed) + n * 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def sample(vertices, faces, cum, S, seed, labels=None):
    """(points float32 [S,3], face int32 [S], labels int32 [S] | None) from `cum`, the inclusive float64 running sum of the areas"""
    v, f, cum = np.asarray(vertices, F32), np.asarray(faces, np.int64), np.asarray(cum, np.float64)
    total = cum[-1]
    points, face = np.empty((S, 3), F32), np.empty(S, np.int32)
    out_label = None if labels is None else np.empty(S, np.int32)
    for s in range(S):
        z0, z1, z2 = (splitmix(seed, 3 * s + k + 1) for k in range(3))
        x = (np.float64(z0 >> 11) * np.float64(2.0 ** -53)) * total
        above = np.nonzero(cum > x)[0]
        fi = int(above[0]) if len(above) else int(np.nonzero(cum == total)[0][0])
        u1, u2 = F32(z1 >> 40) * F32(2.0 ** -24), F32(z2 >> 40) * F32(2.0 ** -24)
        r = np.sqrt(u1)
        a, b, c = F32(1) - r, r * (F32(1) - u2), r * u2
        ia, ib, ic = f[fi]
        points[s] = (a * v[ia] + b * v[ib]) + c * v[ic]
        face[s] = fi
        if labels is not None:
            out_label[s] = labels[(ia if a >= c else ic) if a >= b else (ib if b >= c else ic)]
    return points, face, out_label


# ---- seen -------------------------------------------------------------------------------------------------------------------------------
def seen(vertices, w2c, k, H, W, depth=None, eps=0.0, out=None):
    """uint8 [V]: `out` (or zeros) with a 1 wherever this view sees the vertex; nothing is cleared"""
    p, m = np.asarray(vertices, F32), np.asarray(w2c, F32)
    fx, fy, cx, cy = F32(k[0][0]), F32(k[1][1]), F32(k[0][2]), F32(k[1][2])
    out = np.zeros(len(p), np.uint8) if out is None else out.copy()
    with np.errstate(all="ignore"):
        cam = [((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3] for r in range(3)]
        xc, yc, zc = cam
        ok = zc > 0
        u, v = fx * (xc / zc) + cx, fy * (yc / zc) + cy
        fu, fv = np.floor(u + F32(0.5)), np.floor(v + F32(0.5))
        ok &= (fu >= 0) & (fu < F32(W)) & (fv >= 0) & (fv < F32(H))
        if depth is not None:
            pix = np.where(ok, fv, 0).astype(np.int64) * W + np.where(ok, fu, 0).astype(np.int64)
            d = np.asarray(depth, F32).reshape(-1)[pix]
            ok &= (d > 0) & np.isfinite(d) & (zc <= d + F32(eps))
    out[ok] = 1
    return out


# ---- the grid and the search -------------------------------------------------------------------------------------------------------------
def cell_axis(p, o, c, n):
    with np.errstate(all="ignore"):
        f = np.floor((np.asarray(p, F32) - F32(o)) / F32(c))
        return np.where(f >= n, n - 1, np.where(f > 0, np.nan_to_num(f, nan=0.0, posinf=0.0, neginf=0.0), 0)).astype(np.int32)


def cells(points, origin, c, dims):
    p = np.asarray(points, F32)
    i, j, k = (cell_axis(p[:, a], origin[a], c, dims[a]) for a in range(3))
    return ((k * dims[1] + j) * dims[0] + i).astype(np.int32)


def d2_matrix(queries, points):
    q, p = np.asarray(queries, F32), np.asarray(points, F32)
    with np.errstate(all="ignore"):
        d = q[:, None, :] - p[None, :, :]
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def brute_nn(queries, points):
    """(d2 float32 [N], index int32 [N]): the least d2 over ALL points, the smallest index that reaches it; only a d2 < +inf wins"""
    d2 = d2_matrix(queries, points)
    d2 = np.where(d2 < np.inf, d2, F32(np.inf))      # a NaN fails the comparison
    index = np.argmin(d2, axis=1).astype(np.int32)      # the first occurrence of the minimum
    best = d2[np.arange(len(d2)), index]
    return best.astype(F32), np.where(best < np.inf, index, -1).astype(np.int32)


def grid_of(points, cell):
    """(origin, cell as float32, dims) as hsr_utils.mesh_eval.NearestGrid sizes them"""
    p = np.asarray(points, F32)
    p = p[np.isfinite(p).all(axis=1)].astype(np.float64)
    lo, extent = p.min(axis=0), p.max(axis=0) - p.min(axis=0)
    c = float(cell)
    sides = lambda step: [int(np.floor(e / step)) + 1 for e in extent]
    while max(sides(float(F32(c)))) > 1024 or np.prod([float(s) for s in sides(float(F32(c)))]) > 2 ** 24:
        c *= 1.02
    return tuple(float(F32(o)) for o in lo), float(F32(c)), tuple(sides(float(F32(c))))


def grid_nn(queries, points, origin, c, dims, stats=None):
    """hsr_nn_query's search as a loop: rings of cells around the query's clamped cell, the header's stopping rule"""
    q, p = np.asarray(queries, F32), np.asarray(points, F32)
    X, Y, Z = dims
    cell = cells(p, origin, c, dims)
    order = np.argsort(cell, kind="stable")
    start = np.searchsorted(cell[order], np.arange(X * Y * Z + 1))
    out_d2, out_index = np.full(len(q), np.inf, F32), np.full(len(q), -1, np.int32)
    c32 = F32(c)
    for n in range(len(q)):
        if not np.isfinite(q[n]).all():
            continue
        qi, qj, qk = (int(cell_axis(q[n, a], origin[a], c, dims[a])) for a in range(3))
        best, best_index, r = F32(np.inf), 2 ** 31 - 1, 0
        while True:
            i0, i1, j0, j1, k0, k1 = max(qi - r, 0), min(qi + r, X - 1), max(qj - r, 0), min(qj + r, Y - 1), max(qk - r, 0), min(qk + r, Z - 1)
            spans = []
            for k in range(k0, k1 + 1):
                for j in range(j0, j1 + 1):
                    row = (k * Y + j) * X
                    if k in (qk - r, qk + r) or j in (qj - r, qj + r):
                        spans.append((row + i0, row + i1))
                    else:
                        spans += [(row + i, row + i) for i in (qi - r, qi + r) if 0 <= i < X]
            for a, b in spans:
                members = order[start[a]:start[b + 1]]
                if len(members) == 0:
                    continue
                d2 = d2_matrix(q[n:n + 1], p[members])[0]
                for m, v in zip(members, d2):
                    if v < best or (v == best and m < best_index):
                        best, best_index = v, int(m)
            if r >= 1:
                t = (F32(r) - F32(0.015625)) * c32
                if best <= t * t:
                    break
            if (i0, j0, k0, i1, j1, k1) == (0, 0, 0, X - 1, Y - 1, Z - 1):
                break
            r += 1
        if stats is not None:
            stats.append(r)
        if best < np.inf:
            out_d2[n], out_index[n] = best, best_index
    return out_d2, out_index


# ---- the numbers ------------------------------------------------------------------------------------------------------------------------
def metrics(d2_rec, d2_gt, threshold, gt_labels=None, rec_labels=None, nearest=None, num_classes=None):
    """mesh_metrics from the squared distances (and, for the labels, the nearest rec sample of every gt sample), in float64"""
    da, dc = np.sqrt(np.asarray(d2_rec, np.float64)), np.sqrt(np.asarray(d2_gt, np.float64))
    ra, rc = float((da <= threshold).mean()), float((dc <= threshold).mean())
    out = dict(accuracy=da.mean(), completion=dc.mean(), accuracy_ratio=ra, completion_ratio=rc,
               f_score=2 * ra * rc / (ra + rc) if ra + rc > 0 else 0.0, chamfer=0.5 * (da.mean() + dc.mean()))
    if gt_labels is not None:
        C = int(num_classes)
        confusion = np.zeros((C, C), np.int64)
        for g, m in zip(np.asarray(gt_labels), np.asarray(nearest)):
            pred = rec_labels[m] if m >= 0 else -1
            if 0 <= g < C and 0 <= pred < C:
                confusion[g, pred] += 1
        inter, G, P = np.diag(confusion).astype(np.float64), confusion.sum(axis=1), confusion.sum(axis=0)
        present = (G + P) > 0
        out.update(confusion=confusion, label_accuracy=inter.sum() / max(confusion.sum(), 1),
                   miou=float((inter[present] / (G + P - inter)[present]).mean()) if present.any() else 0.0)
    return out


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------
# the three-face mesh: areas 1, 0 (a repeated point) and 3
TRI_VERTICES = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [5, 5, 5], [3, 0, 0], [3, 2, 0], [0, 2, 0]], F32)
TRI_FACES = np.array([[0, 1, 2], [3, 3, 3], [4, 5, 6]], np.int32)
TRI_LABELS = np.array([10, 11, 12, 13, 14, 15, 16], np.int32)


def nn_fixtures():
    """name -> (queries, targets, cell): the nearest-neighbour cases of the issue"""
    g = np.random.default_rng(7)
    queries = (g.random((1000, 3)) * 1.6 - 0.3).astype(F32)
    targets = g.random((777, 3)).astype(F32)
    flat = targets.copy()
    flat[:, 2] = 0.25
    cluster = np.concatenate([(g.random((300, 3)) * 0.05).astype(F32), np.array([[0.9, 0.9, 0.9], [0.9, 0.0, 0.0], [0.0, 0.9, 0.45]], F32)])
    lattice = np.stack(np.meshgrid(*[np.arange(5) * 0.25] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(F32)
    fine = np.stack(np.meshgrid(*[np.arange(9) * 0.125] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(F32)
    with_nan_q = queries[:70].copy()
    with_nan_q[[3, 40], [0, 2]] = np.nan
    with_nan_q[9] = np.nan
    with_nan_t = targets[:200].copy()
    with_nan_t[[0, 17], [1, 0]] = np.nan
    with_nan_t[5] = np.nan
    c = 0.1
    # a target 0.9 c away in the query's own cell and another 0.1 c away across the cell's face: the query stands at 0.05 c in cell 1
    hand_q = np.array([[1.05 * c, 0.5 * c, 0.5 * c]], F32)
    hand_t = np.array([[1.95 * c, 0.5 * c, 0.5 * c], [0.95 * c, 0.5 * c, 0.5 * c], [0.0, 0.0, 0.0], [3 * c, c, c]], F32)
    return {
        "uniform_c0.1": (queries, targets, 0.1),
        "uniform_c0.37": (queries, targets, 0.37),
        "flat_Z1": (queries, flat, 0.1),
        "cluster_far": (queries[:300], cluster, 0.05),
        "lattice_twice": (fine, np.concatenate([lattice, lattice]), 0.25),
        "M1": (queries[:130], targets[:1], 0.1),
        "N1": (queries[:1], targets, 0.1),
        "nan_query": (with_nan_q, targets, 0.1),
        "nan_target": (queries[:130], with_nan_t, 0.1),
        "hand_first_hit": (hand_q, hand_t, c),
    }


def unit_square(z=0.0, n=4):
    """a unit square at height z as an n x n grid of quads, two triangles each: (vertices, faces)"""
    t = np.linspace(0, 1, n + 1)
    x, y = np.meshgrid(t, t, indexing="xy")
    vertices = np.stack([x.reshape(-1), y.reshape(-1), np.full(x.size, z)], axis=1).astype(F32)
    quad = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).reshape(-1)
    faces = np.concatenate([np.stack([quad, quad + 1, quad + n + 2], 1), np.stack([quad, quad + n + 2, quad + n + 1], 1)]).astype(np.int32)
    return vertices, faces
