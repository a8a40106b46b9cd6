"""The numpy restatement of include/align/hsr_mesh_align.h and of hsr_utils.mesh_align for the tests: the float32 transform chain rounded
once per operation, mesh_eval_ref.brute_nn on the transformed points, the cap, the 17 sums by math.fsum (exact, so the device's sums are
held against the correctly rounded value), rigid_from_sums, the ICP loop in float64 (its nearest neighbours from a KD-tree: the loop is
the reference for what ICP reaches on a scene, not for a pass's bits), the trajectory alignment, and the scene both suites share."""
import math

import numpy as np

import mesh_eval_ref as E

F32 = np.float32
SUMS = 17


# ---- one pass ---------------------------------------------------------------------------------------------------------------------------
def transform32(points, T):
    """the header's chain: x' = ((m00 * x + m01 * y) + m02 * z) + m03 in float32, every operation rounded once"""
    p, m = np.asarray(points, F32), np.asarray(T, np.float64)[:3].astype(F32)
    with np.errstate(all="ignore"):
        return np.stack([((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3] for r in range(3)], axis=1).astype(F32)


def terms(moved, targets, d2, index):
    """[n,17] float64: the terms of the sums, one row per point with a correspondence"""
    has = index >= 0
    p, q = moved[has].astype(np.float64), np.asarray(targets, F32)[index[has]].astype(np.float64)
    return np.concatenate([np.ones((len(p), 1)), p, q, (p[:, :, None] * q[:, None, :]).reshape(len(p), 9), d2[has].astype(np.float64)[:, None]],
                          axis=1)


def step(source, targets, T, max_dist):
    """(d2 float32 [N], index int32 [N], sums float64 [17] by fsum, the sums of the terms' absolute values): hsr_icp_step by brute
    force"""
    moved = transform32(source, T)
    d2, index = E.brute_nn(moved, targets) if len(moved) else (np.zeros(0, F32), np.zeros(0, np.int32))
    m2 = F32(max_dist) * F32(max_dist)
    has = (index >= 0) & (d2 <= m2)
    d2, index = np.where(has, d2, F32(np.inf)).astype(F32), np.where(has, index, -1).astype(np.int32)
    t = terms(moved, targets, d2, index)
    sums = np.array([math.fsum(t[:, k]) for k in range(SUMS)], np.float64)
    return d2, index, sums, np.abs(t).sum(axis=0)


def rigid_from_sums(s):
    s = np.asarray(s, np.float64)
    n = s[0]
    if not n >= 3:
        raise ValueError("fewer than three correspondences")
    mp, mq = s[1:4] / n, s[4:7] / n
    W = s[7:16].reshape(3, 3) - n * np.outer(mp, mq)
    U, _d, Vh = np.linalg.svd(W.T)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vh) < 0:
        S[2, 2] = -1
    R = U @ S @ Vh
    return R, mq - R @ mp


def sums_of(p, q):
    """the 17 sums of the pairs (p_i, q_i), float64 [n,3] each, by fsum"""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    d2 = ((p - q) ** 2).sum(axis=1)
    t = np.concatenate([np.ones((len(p), 1)), p, q, (p[:, :, None] * q[:, None, :]).reshape(len(p), 9), d2[:, None]], axis=1)
    return np.array([math.fsum(t[:, k]) for k in range(SUMS)], np.float64)


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------
def icp(source, target, max_dist=0.1, init=None, max_iterations=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """hsr_utils.mesh_align.icp in float64 throughout: the same loop, the same stopping rules, the same dictionary"""
    from scipy.spatial import cKDTree
    src, tgt = np.asarray(source, np.float64), np.asarray(target, np.float64)
    tree = cKDTree(tgt)
    T = np.eye(4) if init is None else np.asarray(init, np.float64).copy()
    previous, iterations, converged = None, 0, False
    while True:
        moved = src @ T[:3, :3].T + T[:3, 3]
        d, index = tree.query(moved)
        has = d <= max_dist
        if has.sum() < 3:
            raise ValueError("fewer than three correspondences")
        s = sums_of(moved[has], tgt[index[has]])
        fitness, rmse = float(s[0]) / len(src), float(np.sqrt(s[16] / s[0]))
        if previous is not None and abs(previous[0] - fitness) < relative_fitness and abs(previous[1] - rmse) < relative_rmse:
            converged = True
            break
        if iterations >= max_iterations:
            break
        R, t = rigid_from_sums(s)
        update = np.eye(4)
        update[:3, :3], update[:3, 3] = R, t
        T = update @ T
        previous, iterations = (fitness, rmse), iterations + 1
    return dict(transform=T, fitness=fitness, inlier_rmse=rmse, iterations=iterations, converged=converged)


def trajectory_alignment(gt_w2cs, est_w2cs):
    centre = lambda m: -m[:3, :3].T @ m[:3, 3]
    pairs = [(centre(np.asarray(g, np.float64)), centre(np.asarray(e, np.float64))) for g, e in zip(gt_w2cs, est_w2cs) if not np.isnan(g).any()]
    R, t = rigid_from_sums(sums_of([p[1] for p in pairs], [p[0] for p in pairs]))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


# ---- the scene of the end-to-end tests -----------------------------------------------------------------------------------------------------
def rotation(axis, degrees):
    """Rodrigues: the rotation by `degrees` about `axis`"""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.radians(degrees)
    return np.eye(3) + np.sin(r) * K + (1 - np.cos(r)) * (K @ K)


def displacement(degrees=3.0, metres=0.03, middle=None):
    """the known motion of the tests: `degrees` about a skew axis through `middle` (default: the room's) and `metres` along another
    skew direction"""
    middle = ROOM_MIDDLE if middle is None else np.asarray(middle, np.float64)
    T = np.eye(4)
    T[:3, :3] = rotation([1.0, 2.0, 3.0], degrees)
    shift = np.array([2.0, -1.0, 2.0]) / 3.0 * metres
    T[:3, 3] = middle - T[:3, :3] @ middle + shift
    return T


def cuboid(lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(lo, hi)[(i >> a) & 1][a] for a in range(3)] for i in range(8)], F32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    return v, f


ROOM = ((0.0, 0.0, 0.0), (2.0, 1.6, 1.2))
ROOM_MIDDLE = np.array([1.0, 0.8, 0.6])
BUMPS = (((0.3, 0.2, 0.0), (0.9, 0.7, 0.45)), ((1.3, 0.9, 0.0), (1.6, 1.4, 0.8)))      # two unequal boxes on the floor, off every symmetry


def room():
    """(vertices float32 [24,3], faces int32 [36,3]): a box room with two unequal bumps, no symmetry"""
    vs, fs, base = [], [], 0
    for lo, hi in (ROOM,) + BUMPS:
        v, f = cuboid(lo, hi)
        vs.append(v)
        fs.append(f + base)
        base += len(v)
    return np.concatenate(vs), np.concatenate(fs)


def room_samples(n, seed):
    """n surface samples of the room by the restatement of the device's sampler (mesh_eval_ref.sample)"""
    v, f = room()
    return E.sample(v, f, np.cumsum(E.areas(v, f).astype(np.float64)), n, seed)[0]


def transform_error(T, want, points):
    """metres: the farthest any of `points` lands under T from where `want` puts it"""
    p = np.asarray(points, np.float64)
    a, b = p @ np.asarray(T)[:3, :3].T + np.asarray(T)[:3, 3], p @ want[:3, :3].T + want[:3, 3]
    return float(np.sqrt(((a - b) ** 2).sum(axis=1)).max())


def apply64(points, T):
    p = np.asarray(points, np.float64)
    return p @ np.asarray(T)[:3, :3].T + np.asarray(T)[:3, 3]


# ---- the fixture of a step, built for the device suite and checked by the CPU suite ------------------------------------------------------
QUARTER = np.array([[0.0, -1.0, 0.0, 0.25], [1.0, 0.0, 0.0, -0.5], [0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 0.0, 1.0]])      # exact in float32
STEP_CELL, STEP_MAX_DIST = 0.25, 0.5


def step_fixture():
    """dict(source [N,3], targets [M,3], cell, max_dist, transform, marks): about 3 000 targets and 2 000 sources, stated in the frame
    the sources reach under QUARTER — a quarter turn and a binary-exact shift, so that the marked points arrive bit for bit where they
    are put — and pulled back through its exact inverse.  marks: name -> source rows.
      bulk      1 700 sources in [-0.5, 3.5)^3 around 2 800 targets in [0, 3)^3: inside and outside the targets' box
      twice     50 sources standing (to a rounding) on targets that occur twice: an exact tie wherever they arrive, the smaller index wins
      exact     a source at exactly max_dist = 0.5 from the lone target (16, 0, 0), offset (0.5, 0, 0): a correspondence
      above     a source one float above 0.5 from the lone target (0, 16, 0): none
      nan       a source with a NaN                          outside   two sources far outside the box, 20 and 30 m: none
      far       200 sources around (15.5, 15.5, 1.5), inside the box and 50 cells from every target: none, and the call returns"""
    g = np.random.default_rng(21)
    bulk_t = (g.random((2800, 3)) * 3).astype(F32)
    targets = np.concatenate([bulk_t, bulk_t[100:150], np.array([[16, 0, 0], [0, 16, 0]], F32)])
    parts = dict(
        bulk=(g.random((1700, 3)) * 4 - 0.5).astype(F32),
        twice=bulk_t[100:150].copy(),
        exact=np.array([[16.5, 0, 0]], F32),
        above=np.array([[np.nextafter(F32(0.5), F32(1)), 16, 0]], F32),
        nan=np.array([[1.0, np.nan, 1.0]], F32),
        outside=np.array([[-20, 1, 1], [1, 30, 1]], F32),
        far=(np.array([15.5, 15.5, 1.5]) + g.random((200, 3)) * 0.4 - 0.2).astype(F32))
    arrived = np.concatenate(list(parts.values()))
    marks, at = {}, 0
    for name, rows in parts.items():
        marks[name] = np.arange(at, at + len(rows))
        at += len(rows)
    inverse = np.linalg.inv(QUARTER)
    source = (arrived.astype(np.float64) @ inverse[:3, :3].T + inverse[:3, 3]).astype(F32)
    return dict(source=source, targets=targets, cell=STEP_CELL, max_dist=STEP_MAX_DIST, transform=QUARTER, marks=marks, arrived=arrived)


def general_transform():
    """a transform with no exact entry: 10 degrees about a skew axis and a shift"""
    T = np.eye(4)
    T[:3, :3] = rotation([3.0, -1.0, 2.0], 10.0)
    T[:3, 3] = [0.07, -0.11, 0.05]
    return T
