"""The two rules of include/shade/hsr_mesh_shade.h restated in numpy for the tests: the vertex normals with float32 crosses, 64-bit
integer sums and the float64 finish; the pictures with one rounding per float32 operation in the header's order and the header's byte
rule; the same normals in plain float64 as what the restatement itself is measured against; the construction of
hsr_utils.mesh_view.orbit_views restated from its docstring; and the scenes both suites share.  The face terms, the camera points and
the depth image come from tests/mesh_depth_ref.py (hsr_mesh_depth.h's restatement).  Nothing here imports the package."""
import numpy as np

import mesh_depth_ref as D

F32 = np.float32
SHADED, COLOUR, NORMALS, LABELS, SCALAR = 0, 1, 2, 3, 4      # HSR_SHADE_*, restated: the CPU suite compares them with the header's
KINDS = {"shaded": SHADED, "colour": COLOUR, "normals": NORMALS, "labels": LABELS, "scalar": SCALAR}
FIX = 2.0 ** 40
LIMIT = F32(65536)


# ---- vertex normals -----------------------------------------------------------------------------------------------------------------------
def face_cross(vertices, tri):
    """cross(B - A, C - A) of a face in float32, one rounding per operation"""
    A, B, C = (np.asarray(vertices, F32)[int(i)] for i in tri)
    with np.errstate(all="ignore"):
        return D.cross(B - A, C - A)


def normals(vertices, faces):
    """float32 [V,3] by the header's rule: 2^40 fixed point, int64 sums (wrap-around included), the float64 finish"""
    v = np.asarray(vertices, F32)
    V = len(v)
    sums = np.zeros((V, 3), np.int64)
    for tri in np.asarray(faces).reshape(-1, 3):
        if not all(0 <= int(i) < V for i in tri):
            continue
        c = face_cross(v, tri)
        if not (np.abs(c) < LIMIT).all():      # a NaN fails
            continue
        q = np.rint(c.astype(np.float64) * FIX).astype(np.int64)      # exact product, halves to even
        for i in tri:
            with np.errstate(over="ignore"):
                sums[int(i)] += q
    d = sums.astype(np.float64) * (1.0 / FIX)
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    with np.errstate(all="ignore"):
        n = (d / length[:, None]).astype(F32)
    return np.where(length[:, None] == 0, F32(0), n).astype(F32)


def normals64(vertices, faces):
    """area-weighted vertex normals in plain float64 on the same float32 inputs: no fixed point, no float32 cross"""
    v = np.asarray(vertices, F32).astype(np.float64)
    f = np.asarray(faces).reshape(-1, 3)
    c = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    out = np.zeros_like(v)
    for k in range(3):
        np.add.at(out, f[:, k], c)
    return out / np.linalg.norm(out, axis=1, keepdims=True)


# ---- the pictures -------------------------------------------------------------------------------------------------------------------------
def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def unit3(n):
    """(n / |n|, ok): ok where 0 < |n| < inf"""
    with np.errstate(all="ignore"):
        length = np.sqrt(dot3(n, n))
        ok = (length > 0) & (length < np.inf)
        return (n / length[..., None]).astype(F32), ok


def code(t):
    """HSR_EXPORT_COLOR's byte of a float colour: clamp (a NaN gives 0), one product by 255, halves to even"""
    t = np.asarray(t, F32)
    with np.errstate(all="ignore"):
        c = np.where(t > 0, np.where(t < 1, t, F32(1)), F32(0)).astype(F32)
        return np.rint(c * F32(255)).astype(np.uint8)


def pixel_terms(vertices, faces, w2c, k, H, W, face_image):
    """what all jobs of a pixel share, over the flat index: dict of hit bool [N], idx int [N,3], b float32 [N,3] (the weights), z [N],
    p [N,3], v [N,3], nf [N,3]; rows where hit is False hold anything"""
    fx, fy, cx, cy = D.pinhole(k)
    cam = D.camera_points(vertices, w2c)
    V = len(cam)
    tris = np.asarray(faces).reshape(-1, 3)
    F = len(tris)
    ok = np.zeros(F + 1, bool)
    n3 = np.zeros((F + 1, 3, 3), F32)
    det = np.ones(F + 1, F32)
    nf = np.zeros((F + 1, 3), F32)
    idx = np.zeros((F + 1, 3), np.int64)
    for f, tri in enumerate(tris):
        terms = D.face_terms(cam, V, tri)
        if terms is None:
            continue
        nA, nB, nC, dt, A, B, C = terms
        ok[f], n3[f], det[f], idx[f] = True, np.stack([nA, nB, nC]), dt, tri
        with np.errstate(all="ignore"):
            g = D.cross(B - A, C - A)
        u, good = unit3(g)
        nf[f] = u if good else np.array([0, 0, -1], F32)
    image = np.asarray(face_image).reshape(-1).astype(np.int64)
    N = H * W
    assert image.shape == (N,)
    inside = (image >= 0) & (image < F)
    f = np.where(inside, image, F)      # row F: a face that takes no part
    i = np.arange(N)
    x, y = (i % W).astype(F32), (i // W).astype(F32)
    with np.errstate(all="ignore"):
        rx, ry = (x - cx) / fx, (y - cy) / fy
        w = np.stack([(rx * n3[f, j, 0] + ry * n3[f, j, 1]) + n3[f, j, 2] for j in range(3)], axis=1)
        s = (w[:, 0] + w[:, 1]) + w[:, 2]
        b = (w / s[:, None]).astype(F32)
        z = (det[f] / s).astype(F32)
        hit = ok[f] & (s != 0) & (z > 0) & (z < np.inf)
        p = np.stack([z * rx, z * ry, z], axis=1).astype(F32)
        length = np.sqrt(dot3(p, p))
        v = (-p / length[:, None]).astype(F32)
    return dict(hit=hit, idx=idx[f], b=b, z=z, p=p, v=v, nf=nf[f], s=s)


def shading_normal(terms, w2c, vertex_normals):
    """float32 [N,3]: the header's shading normal for vertex_normals (None: flat), turned towards the camera"""
    n = terms["nf"]
    if vertex_normals is not None:
        m = np.asarray(w2c, F32)
        vn = np.asarray(vertex_normals, F32)
        b = terms["b"]
        with np.errstate(all="ignore"):
            r = []
            for corner in range(3):
                w = vn[terms["idx"][:, corner]]
                r.append(np.stack([(m[c][0] * w[:, 0] + m[c][1] * w[:, 1]) + m[c][2] * w[:, 2] for c in range(3)], axis=1))
            t = np.stack([(b[:, 0] * r[0][:, c] + b[:, 1] * r[1][:, c]) + b[:, 2] * r[2][:, c] for c in range(3)], axis=1).astype(F32)
        u, ok = unit3(t)
        n = np.where(ok[:, None], u, n).astype(F32)
    with np.errstate(all="ignore"):
        flip = dot3(n, terms["p"]) > 0
    return np.where(flip[:, None], -n, n).astype(F32)


def job(kind, normals=None, attr=None, table=None, lo=0.0, hi=1.0, ambient=0.25, albedo=(0.8, 0.8, 0.8), background=(255, 255, 255), lit=True):
    return dict(kind=KINDS.get(kind, kind), normals=normals, attr=attr, table=table, lo=lo, hi=hi, ambient=ambient, albedo=albedo,
                background=background, lit=lit)


def lit_bytes(rows, lit, shade):
    """uint8 [N,3] table colours, lit or as they are"""
    if not lit:
        return rows
    with np.errstate(all="ignore"):
        return code(rows.astype(F32) / F32(255) * shade[:, None])


def shade(vertices, faces, w2c, k, H, W, face_image, jobs, terms=None):
    """the pictures of the jobs, a list of uint8 [H,W,3], by the header's rule"""
    terms = pixel_terms(vertices, faces, w2c, k, H, W, face_image) if terms is None else terms
    hit, b, idx = terms["hit"], terms["b"], terms["idx"]
    out = []
    for j in jobs:
        n = shading_normal(terms, w2c, j["normals"])
        ambient = F32(j["ambient"])
        with np.errstate(all="ignore"):
            shade_ = ambient + (F32(1) - ambient) * np.abs(dot3(n, terms["v"]))
            if j["kind"] == SHADED:
                rgb = code(np.stack([F32(a) * shade_ for a in j["albedo"]], axis=1))
            elif j["kind"] == COLOUR:
                c = np.asarray(j["attr"], np.uint8)[idx].astype(F32)      # [N, corner, channel]
                t = ((b[:, 0, None] * c[:, 0] + b[:, 1, None] * c[:, 1]) + b[:, 2, None] * c[:, 2]) / F32(255)
                rgb = code(t * shade_[:, None] if j["lit"] else t)
            elif j["kind"] == NORMALS:
                rgb = code(np.stack([n[:, 0] * F32(0.5) + F32(0.5), -n[:, 1] * F32(0.5) + F32(0.5), -n[:, 2] * F32(0.5) + F32(0.5)], axis=1))
            elif j["kind"] == LABELS:
                table = np.asarray(j["table"], np.uint8)
                slot = np.zeros(len(b), np.int64)
                slot = np.where(b[:, 1] > b[:, 0], 1, slot)
                slot = np.where(b[:, 2] > b[np.arange(len(b)), slot], 2, slot)
                label = np.asarray(j["attr"], np.int64)[idx[np.arange(len(b)), slot]]
                ok = (label >= 0) & (label < len(table))
                rgb = np.where(ok[:, None], lit_bytes(table[np.where(ok, label, 0)], j["lit"], shade_), np.uint8(0)).astype(np.uint8)
            elif j["kind"] == SCALAR:
                table = np.asarray(j["table"], np.uint8)
                assert len(table) == 256
                s = np.asarray(j["attr"], F32)[idx]
                t = (b[:, 0] * s[:, 0] + b[:, 1] * s[:, 1]) + b[:, 2] * s[:, 2]
                u = (t - F32(j["lo"])) / (F32(j["hi"]) - F32(j["lo"]))
                u = np.where(u > 0, np.where(u < 1, u, F32(1)), F32(0)).astype(F32)
                rgb = lit_bytes(table[(u * F32(255)).astype(np.int64)], j["lit"], shade_)
            else:
                raise ValueError(j["kind"])
        rgb = np.where(hit[:, None], rgb, np.asarray(j["background"], np.uint8)[None, :]).astype(np.uint8)
        out.append(rgb.reshape(H, W, 3))
    return out


# ---- orbit views --------------------------------------------------------------------------------------------------------------------------
def orbit_view(lo, hi, n, i, elevation_deg=30.0, distance=None, up=None):
    """(eye, centre, distance, u) of view i, from the docstring of hsr_utils.mesh_view.orbit_views"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    centre = (lo + hi) / 2
    distance = 1.5 * np.linalg.norm(hi - lo) if distance is None else distance
    u = np.array([0.0, -1.0, 0.0]) if up is None else np.asarray(up, np.float64)
    u = u / np.linalg.norm(u)
    e = np.eye(3)[int(np.argmin(np.abs(u)))]
    a = e - (e @ u) * u
    a = a / np.linalg.norm(a)
    b = np.cross(u, a)
    phi, theta = 2 * np.pi * i / n, np.deg2rad(elevation_deg)
    eye = centre + distance * (np.cos(theta) * (np.cos(phi) * a + np.sin(phi) * b) + np.sin(theta) * u)
    return eye, centre, distance, u


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------
def sphere(levels=2, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """(vertices float32 [V,3], faces int32 [F,3]): an octahedron subdivided `levels` times onto the sphere; 128 faces and 66 vertices at
    levels = 2, wound so that cross(B - A, C - A) points outwards"""
    v = [np.array(p, np.float64) for p in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(levels):
        mid, nf = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            nf += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius + np.asarray(centre)).astype(F32), np.array(f, np.int32)


def fan(n=2000, seed=0):
    """(vertices float32 [n+2,3], faces int32 [n,3]): n faces round one hub (vertex 0), the rim a jittered circle: every face's
    contribution meets at the hub"""
    rng = np.random.default_rng(seed)
    phi = np.linspace(0, 2 * np.pi, n + 1)
    rim = np.stack([np.cos(phi), np.sin(phi), rng.uniform(-0.2, 0.2, n + 1)], axis=1) * rng.uniform(0.8, 1.2, (n + 1, 1))
    vertices = np.concatenate([[[0.0, 0.0, 0.5]], rim]).astype(F32)
    faces = np.stack([np.zeros(n, np.int64), np.arange(1, n + 1), np.arange(2, n + 2)], axis=1).astype(np.int32)
    return vertices, faces


def take_no_part(vertices, faces):
    """the random_faces scene with the take-no-part clauses of both rules in it: faces 5, 17, 40 with out-of-range indices, 60 and 61
    degenerate, 90 with a coordinate of 1e30 at its first corner (both edges from it are huge, so cross(B - A, C - A) is not finite; in
    camera space its crosses are still finite: hsr_mesh_depth takes it) and 91 with one of 3e38 (its camera-space crosses are not
    finite either: no rule takes it); returns copies"""
    v, f = np.array(vertices, F32), np.array(faces, np.int32)
    V = len(v)
    f[5] = [f[5][0], V, f[5][2]]
    f[17] = [-1, f[17][1], f[17][2]]
    f[40] = [f[40][0], f[40][1], 2 ** 31 - 1]
    f[60] = [f[60][0], f[60][0], f[60][2]]      # two equal corners
    f[61] = [f[61][1], f[61][1], f[61][1]]
    v[f[90][0]][0] = F32(1e30)
    v[f[91][0]][0] = F32(3e38)
    return v, f


def attributes(V, seed=0, n_labels=7):
    """(rgb uint8 [V,3], labels int32 [V], scalar float32 [V]) for a mesh of V vertices"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (V, 3)).astype(np.uint8), rng.integers(0, n_labels, V).astype(np.int32), rng.uniform(-0.5, 1.5, V).astype(F32)


def table(n, seed=0):
    return np.random.default_rng(1000 + seed).integers(0, 256, (n, 3)).astype(np.uint8)


def shading_normals64(vertices, faces, w2c, k, H, W, face_image, vertex_normals):
    """float64 [N,3] (NaN rows where nothing is hit) and the hit points float64 [N,3]: the smooth shading normal by the header's
    formulas in plain float64 on the same float32 inputs, with float64 vertex normals (normals64), turned towards the camera"""
    fx, fy, cx, cy = (float(x) for x in D.pinhole(k))
    cam = D.camera_points(vertices, w2c, np.float64)
    rot = np.asarray(w2c, F32).astype(np.float64)[:3, :3]
    tris = np.asarray(faces).reshape(-1, 3)
    image = np.asarray(face_image).reshape(-1)
    n = np.full((H * W, 3), np.nan)
    p = np.full((H * W, 3), np.nan)
    for i in np.flatnonzero((image >= 0) & (image < len(tris))):
        terms = D.face_terms(cam, len(cam), tris[image[i]])
        if terms is None:
            continue
        nA, nB, nC, det = terms[:4]
        ray = np.array([(i % W - cx) / fx, (i // W - cy) / fy, 1.0])
        w = np.array([ray @ nA, ray @ nB, ray @ nC])
        b = w / w.sum()
        p[i] = ray * (det / w.sum())
        t = rot @ (b @ np.asarray(vertex_normals, np.float64)[tris[image[i]]])
        t = t / np.linalg.norm(t)
        n[i] = -t if t @ p[i] > 0 else t
    return n, p
