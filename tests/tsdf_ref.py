"""A numpy float32 restatement of include/ext/hsr_tsdf.h, rule by rule, vectorised over the volume: what hsr_tsdf_integrate,
hsr_tsdf_count / hsr_tsdf_faces and hsr_tsdf_vertices must produce.  Every operation is one float32 operation (numpy rounds each once;
no value here is ever a float64), in the header's order, so integrate and vertices are expected BIT FOR BIT; the faces as a set of
oriented triangles (the device's emission order is its own).  Written from the header alone: the C code is not read."""
import numpy as np

F = np.float32
# the six Kuhn tetrahedra: corner numbers dx + 2 dy + 4 dz of v0..v3 for the axis orders xyz, xzy, yxz, yzx, zxy, zyx, and their orientations
TETS = ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))
TET_SIGN = (1, -1, -1, 1, 1, -1)


def tet_orientation(tet):
    """det[v1 - v0, v2 - v0, v3 - v0] of a tetrahedron given by corner numbers: what TET_SIGN must equal"""
    p = np.array([[(c >> a) & 1 for a in range(3)] for c in tet], np.int64)
    return int(round(np.linalg.det((p[1:] - p[0]).astype(np.float64))))


class Volume:
    """the state of include/ext/hsr_tsdf.h as numpy arrays, flat in lin = (k * Y + j) * X + i"""

    def __init__(self, origin, dims, h, trunc, max_weight, color=True, labels=False):
        self.X, self.Y, self.Z = (int(d) for d in dims)
        self.origin = tuple(F(o) for o in origin)
        self.h, self.trunc, self.max_weight = F(h), F(trunc), F(max_weight)
        N = self.N = self.X * self.Y * self.Z
        self.tsdf, self.weight = np.ones(N, F), np.zeros(N, F)
        self.color, self.cweight = (np.zeros((3, N), F), np.zeros(N, F)) if color else (None, None)
        self.best, self.label = (np.full(N, np.inf, F), np.full(N, -1, np.int32)) if labels else (None, None)

    def copy(self):
        import copy
        return copy.deepcopy(self)

    def ijk(self):
        lin = np.arange(self.N, dtype=np.int64)
        return lin % self.X, (lin // self.X) % self.Y, lin // (self.X * self.Y)

    def points(self, i, j, k):
        ox, oy, oz = self.origin
        return ox + self.h * i.astype(F), oy + self.h * j.astype(F), oz + self.h * k.astype(F)

    def state(self):
        return {n: getattr(self, n) for n in ("tsdf", "weight", "color", "cweight", "best", "label") if getattr(self, n) is not None}


def integrate(vol, depth, w2c, k, image=None, labels=None, opacity=None, sil_thres=0.0, depth_max=0.0):
    """one view into `vol`, in place.  depth [H,W] float32, w2c [4,4], k [3,3]; image [3,H,W] float32, labels [H,W] int64, opacity [H,W]"""
    H, W = depth.shape
    m = np.asarray(w2c, F)
    fx, fy, cx, cy = F(k[0][0]), F(k[1][1]), F(k[0][2]), F(k[1][2])
    depth = np.asarray(depth, F).reshape(-1)
    px, py, pz = vol.points(*vol.ijk())
    with np.errstate(all="ignore"):
        xc = ((m[0, 0] * px + m[0, 1] * py) + m[0, 2] * pz) + m[0, 3]
        yc = ((m[1, 0] * px + m[1, 1] * py) + m[1, 2] * pz) + m[1, 3]
        zc = ((m[2, 0] * px + m[2, 1] * py) + m[2, 2] * pz) + m[2, 3]
        ok = zc > 0
        u = fx * (xc / zc) + cx
        v = fy * (yc / zc) + cy
        fu, fv = np.floor(u + F(0.5)), np.floor(v + F(0.5))
        assert fu.dtype == F and zc.dtype == F
        ok &= (fu >= 0) & (fu < F(W)) & (fv >= 0) & (fv < F(H))      # in float: a NaN compares false
        pix = np.where(ok, fv, 0).astype(np.int64) * W + np.where(ok, fu, 0).astype(np.int64)
        d = depth[pix]
        ok &= (d > 0) & np.isfinite(d)
        if F(depth_max) > 0:
            ok &= ~(d > F(depth_max))
        if opacity is not None:
            ok &= np.asarray(opacity, F).reshape(-1)[pix] > F(sil_thres)
        sdf = d - zc
        ok &= ~(sdf < -vol.trunc)
        t = np.fmin(F(1), sdf / vol.trunc)
        w = vol.weight
        new_tsdf = (vol.tsdf * w + t) / (w + F(1))
        new_weight = np.fmin(w + F(1), vol.max_weight)
        assert new_tsdf.dtype == F and sdf.dtype == F
        band = ok & (np.abs(sdf) <= vol.trunc)
        if image is not None:
            cw = vol.cweight
            img = np.asarray(image, F).reshape(3, -1)
            for c in range(3):
                vol.color[c] = np.where(band, (vol.color[c] * cw + img[c][pix]) / (cw + F(1)), vol.color[c])
            vol.cweight = np.where(band, np.fmin(cw + F(1), vol.max_weight), cw)
        if labels is not None:
            closer = band & (np.abs(sdf) < vol.best)
            vol.best = np.where(closer, np.abs(sdf), vol.best)
            vol.label = np.where(closer, np.asarray(labels, np.int64).reshape(-1)[pix].astype(np.int32), vol.label)
        vol.tsdf = np.where(ok, new_tsdf, vol.tsdf)
        vol.weight = np.where(ok, new_weight, vol.weight)
    return vol


# ---- the surface ----------------------------------------------------------------------------------------------------------------------------
def _corner_lin(lin, corner, X, Y):
    return lin + (corner & 1) + ((corner >> 1) & 1) * X + ((corner >> 2) & 1) * X * Y


def _edge_key(lin, tet, p, q, X, Y):
    lo, hi = min(p, q), max(p, q)
    return _corner_lin(lin, tet[lo], X, Y) * 8 + (tet[hi] ^ tet[lo])


def _permutation_sign(order):
    inv = sum(1 for a in range(len(order)) for b in range(a + 1, len(order)) if order[a] > order[b])
    return -1 if inv & 1 else 1


def face_keys(X, Y, Z, tsdf, weight):
    """int64 [T,3]: the edge keys of every triangle, grouped by tetrahedron and case (NOT the device's emission order)"""
    tsdf, weight = np.asarray(tsdf, F).reshape(-1), np.asarray(weight, F).reshape(-1)
    lin = np.arange(X * Y * Z, dtype=np.int64)
    i, j, k = lin % X, (lin // X) % Y, lin // (X * Y)
    lin = lin[(i + 1 < X) & (j + 1 < Y) & (k + 1 < Z)]
    if lin.size == 0:
        return np.zeros((0, 3), np.int64)
    corners = [_corner_lin(lin, c, X, Y) for c in range(8)]
    seen = np.all([weight[c] > 0 for c in corners], axis=0)
    lin, corners = lin[seen], [c[seen] for c in corners]
    inside = [tsdf[c] < 0 for c in corners]
    out = []
    for tet, s in zip(TETS, TET_SIGN):
        flags = [inside[c] for c in tet]
        mask = sum(f.astype(np.int64) << q for q, f in enumerate(flags))
        for case in range(1, 15):
            cube = lin[mask == case]
            if cube.size == 0:
                continue
            ins = [q for q in range(4) if (case >> q) & 1]
            outs = [q for q in range(4) if not (case >> q) & 1]
            key = lambda p, q: _edge_key(cube, tet, p, q, X, Y)
            if len(ins) == 2:
                (a, b), (c, d) = ins, outs
                quad = [key(a, c), key(a, d), key(b, d), key(b, c)]
                if s * _permutation_sign((a, b, c, d)) < 0:
                    quad = quad[::-1]
                quad = np.stack(quad, axis=1)
                first = np.argmin(quad, axis=1)
                rows = np.arange(cube.size)
                q = [quad[rows, (first + r) % 4] for r in range(4)]
                out += [np.stack([q[0], q[1], q[2]], axis=1), np.stack([q[0], q[2], q[3]], axis=1)]
            else:
                p = ins[0] if len(ins) == 1 else outs[0]
                rest = [q for q in range(4) if q != p]
                away = s * _permutation_sign([p] + rest) > 0      # the triangle pq1, pq2, pq3 faces away from p
                if away != (len(ins) == 1):
                    rest = [rest[0], rest[2], rest[1]]
                out.append(np.stack([key(p, q) for q in rest], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 3), np.int64)


def cube_counts(X, Y, Z, tsdf, weight):
    """int32 [X*Y*Z]: the triangles of every cube, from the number of inside vertices of each tetrahedron (1 or 3: one, 2: two)"""
    tsdf, weight = np.asarray(tsdf, F).reshape(-1), np.asarray(weight, F).reshape(-1)
    counts = np.zeros(X * Y * Z, np.int32)
    lin = np.arange(X * Y * Z, dtype=np.int64)
    i, j, k = lin % X, (lin // X) % Y, lin // (X * Y)
    lin = lin[(i + 1 < X) & (j + 1 < Y) & (k + 1 < Z)]
    if lin.size == 0:
        return counts
    corners = [_corner_lin(lin, c, X, Y) for c in range(8)]
    seen = np.all([weight[c] > 0 for c in corners], axis=0)
    for tet in TETS:
        n = sum((tsdf[corners[c]] < 0).astype(np.int32) for c in tet)
        counts[lin] += np.where(seen, np.where(n == 2, 2, np.where((n == 1) | (n == 3), 1, 0)), 0).astype(np.int32)
    return counts


def vertices(vol, keys):
    """(positions float32 [V,3], rgb uint8 [V,3] | None, labels int32 [V] | None) of the edge keys `keys` (int64 [V])"""
    keys = np.asarray(keys, np.int64)
    lo, direction = keys >> 3, keys & 7
    X, Y = vol.X, vol.Y
    hi = lo + (direction & 1) + ((direction >> 1) & 1) * X + ((direction >> 2) & 1) * X * Y
    i, j, k = lo % X, (lo // X) % Y, lo // (X * Y)
    p0 = vol.points(i, j, k)
    p1 = vol.points(i + (direction & 1), j + ((direction >> 1) & 1), k + ((direction >> 2) & 1))
    s0, s1 = vol.tsdf[lo], vol.tsdf[hi]
    with np.errstate(all="ignore"):
        t = s0 / (s0 - s1)
        pos = np.stack([a + t * (b - a) for a, b in zip(p0, p1)], axis=1)
        assert pos.dtype == F
        rgb = None
        if vol.color is not None:
            has0, has1 = vol.cweight[lo] > 0, vol.cweight[hi] > 0
            rgb = np.zeros((keys.size, 3), np.uint8)
            for c in range(3):
                c0, c1 = vol.color[c][lo], vol.color[c][hi]
                mix = np.where(has0 & has1, c0 + t * (c1 - c0), np.where(has0, c0, np.where(has1, c1, F(0.5))))
                clamped = np.where(mix > 0, np.where(mix < 1, mix, F(1)), F(0)).astype(F)      # a NaN fails mix > 0
                rgb[:, c] = np.rint(clamped * F(255)).astype(np.uint8)
        labels = None if vol.label is None else np.where(np.abs(s0) <= np.abs(s1), vol.label[lo], vol.label[hi]).astype(np.int32)
    return pos, rgb, labels


def extract(vol):
    """(vertices [V,3], faces int32 [F,3], rgb | None, labels | None, keys int64 [V]): torch.unique's sorted keys name the vertices"""
    tri = face_keys(vol.X, vol.Y, vol.Z, vol.tsdf, vol.weight)
    keys, inverse = np.unique(tri.reshape(-1), return_inverse=True)
    pos, rgb, labels = vertices(vol, keys)
    return pos, inverse.reshape(-1, 3).astype(np.int32), rgb, labels, keys


# ---- what the tests ask of a mesh -------------------------------------------------------------------------------------------------------------
def canonical_faces(faces):
    """the faces as a sorted list of triples, each rotated (never flipped) to start with its smallest index"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    first = np.argmin(f, axis=1)
    rows = np.arange(f.shape[0])
    f = np.stack([f[rows, (first + r) % 3] for r in range(3)], axis=1)
    return f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))]


def topology(faces):
    """(closed and manifold: every undirected edge in exactly two faces, once in each direction; V - E + F over the used vertices)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    uniq_directed = np.unique(directed, axis=0)
    undirected, counts = np.unique(np.sort(directed, axis=1), axis=0, return_counts=True)
    reversed_present = len(np.unique(np.concatenate([uniq_directed, uniq_directed[:, ::-1]]), axis=0)) == len(uniq_directed)
    closed = bool(len(uniq_directed) == len(directed) and (counts == 2).all() and reversed_present and (f[:, 0] != f[:, 1]).all()
                  and (f[:, 1] != f[:, 2]).all() and (f[:, 2] != f[:, 0]).all())
    return closed, int(len(np.unique(f)) - len(undirected) + len(f))


def signed_volume(pos, faces):
    p = np.asarray(pos, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def sphere_volume(dims, h, centre, radius, trunc, color=False, labels=False):
    """a volume whose tsdf is the clamped distance to a sphere (negative inside), every point observed"""
    vol = Volume((0.0, 0.0, 0.0), dims, h, trunc, 64.0, color=color, labels=labels)
    px, py, pz = vol.points(*vol.ijk())
    dist = np.sqrt((px - F(centre[0])) ** 2 + (py - F(centre[1])) ** 2 + (pz - F(centre[2])) ** 2).astype(F) - F(radius)
    vol.tsdf = np.clip(dist / F(trunc), F(-1), F(1)).astype(F)
    vol.weight = np.ones(vol.N, F)
    return vol


def same_floats(a, b):
    """bit-equal, a NaN matching any NaN (the payload of a NaN an operation makes is the hardware's)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
