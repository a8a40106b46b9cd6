"""The rule of include/recon/hsr_mesh_depth.h restated in numpy for the tests: float32 with one rounding per operation in the header's
order, the box of a face included, and the 64-bit key minimum; the same formulas in float64 on the same float32 inputs, without the box,
as what the restatement itself is measured against; the construction of hsr_utils.mesh_depth.virtual_views restated from its docstring;
and the scenes both suites share.  Nothing here imports the package."""
import numpy as np

F32 = np.float32
EMPTY = np.uint64(2 ** 64 - 1)
SMALL_BOX = 255     # HSR_MESH_DEPTH_SMALL_BOX, restated: the tests compare it with the header's and the module's


def pinhole(k):
    k = np.asarray(k, np.float64)
    return F32(k[0][0]), F32(k[1][1]), F32(k[0][2]), F32(k[1][2])


def camera_points(vertices, w2c, dtype=F32):
    """xc = ((m00 * px + m01 * py) + m02 * pz) + m03, likewise yc and zc"""
    m = np.asarray(w2c, F32).astype(dtype)
    p = np.asarray(vertices, F32).astype(dtype)
    with np.errstate(all="ignore"):
        return np.stack([((m[r][0] * p[:, 0] + m[r][1] * p[:, 1]) + m[r][2] * p[:, 2]) + m[r][3] for r in range(3)], axis=1)


def cross(P, Q):
    return np.array([P[1] * Q[2] - P[2] * Q[1], P[2] * Q[0] - P[0] * Q[2], P[0] * Q[1] - P[1] * Q[0]], dtype=P.dtype)


def face_terms(cam, V, tri):
    """(nA, nB, nC, det, A, B, C) of a face, or None when it takes no part"""
    if not all(0 <= int(i) < V for i in tri):
        return None
    A, B, C = cam[int(tri[0])], cam[int(tri[1])], cam[int(tri[2])]
    with np.errstate(all="ignore"):
        if not (np.isfinite(A).all() and np.isfinite(B).all() and np.isfinite(C).all()):
            return None
        nA, nB, nC = cross(B, C), cross(C, A), cross(A, B)
        if not (np.isfinite(nA).all() and np.isfinite(nB).all() and np.isfinite(nC).all()):
            return None
        det = (A[0] * nA[0] + A[1] * nA[1]) + A[2] * nA[2]
    if not np.isfinite(det) or det == 0:
        return None
    return nA, nB, nC, det, A, B, C


def face_box(A, B, C, fx, fy, cx, cy, H, W, near):
    """(x0, x1, y0, y1) inclusive, or None when the box is empty or all three corners lie nearer than near"""
    if A[2] < near and B[2] < near and C[2] < near:
        return None      # the face takes no part
    if A[2] < near or B[2] < near or C[2] < near:
        return 0, W - 1, 0, H - 1
    with np.errstate(all="ignore"):
        u = [fx * (P[0] / P[2]) + cx for P in (A, B, C)]
        v = [fy * (P[1] / P[2]) + cy for P in (A, B, C)]
        x0, x1 = np.floor(min(u)) - F32(1), np.ceil(max(u)) + F32(1)
        y0, y1 = np.floor(min(v)) - F32(1), np.ceil(max(v)) + F32(1)
    xe, ye = F32(W - 1), F32(H - 1)
    if not (x1 >= 0 and x0 <= xe and y1 >= 0 and y0 <= ye):
        return None
    return int(max(x0, F32(0))), int(min(x1, xe)), int(max(y0, F32(0))), int(min(y1, ye))


def render(vertices, faces, w2c, k, H, W, near=0.01, boxes=None):
    """(depth float32 [H,W], face int32 [H,W]) by the header's rule.  boxes: a list that receives the number of pixels of every face's
    box (0 for a face that takes no part or has an empty box)."""
    fx, fy, cx, cy = pinhole(k)
    near = F32(near)
    cam = camera_points(vertices, w2c)
    V = len(cam)
    key = np.full((H, W), EMPTY)
    for f, tri in enumerate(np.asarray(faces).reshape(-1, 3)):
        terms = face_terms(cam, V, tri)
        box = None if terms is None else face_box(*terms[4:], fx, fy, cx, cy, H, W, near)
        if boxes is not None:
            boxes.append(0 if box is None else (box[1] - box[0] + 1) * (box[3] - box[2] + 1))
        if box is None:
            continue
        nA, nB, nC, det = terms[:4]
        x0, x1, y0, y1 = box
        rx = ((np.arange(x0, x1 + 1).astype(F32) - cx) / fx)[None, :]
        ry = ((np.arange(y0, y1 + 1).astype(F32) - cy) / fy)[:, None]
        with np.errstate(all="ignore"):
            w = [(rx * n[0] + ry * n[1]) + n[2] for n in (nA, nB, nC)]
            s = (w[0] + w[1]) + w[2]
            inside = (w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0) if det > 0 else (w[0] <= 0) & (w[1] <= 0) & (w[2] <= 0)
            z = (det / s).astype(F32)
            hit = inside & (s != 0) & np.isfinite(z) & (z >= near)
        new = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
        part = key[y0:y1 + 1, x0:x1 + 1]
        key[y0:y1 + 1, x0:x1 + 1] = np.where(hit & (new < part), new, part)
    hit = key != EMPTY
    depth = np.where(hit, (key >> np.uint64(32)).astype(np.uint32).view(F32), F32(0)).astype(F32)
    face = np.where(hit, (key & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return depth, face


def render64(vertices, faces, w2c, k, H, W, near=0.01):
    """the same formulas in float64 on the same float32 inputs, every face that takes part tested at every pixel: (depth float64 [H,W], face int32
    [H,W], margin float64 [H,W]) — margin is the winner's smallest barycentric weight min(wA, wB, wC) / s, NaN where nothing hits"""
    fx, fy, cx, cy = (float(v) for v in pinhole(k))
    cam = camera_points(vertices, w2c, np.float64)
    rx = ((np.arange(W) - cx) / fx)[None, :]
    ry = ((np.arange(H) - cy) / fy)[:, None]
    depth = np.full((H, W), np.inf)
    face = np.full((H, W), -1, np.int32)
    margin = np.full((H, W), np.nan)
    for f, tri in enumerate(np.asarray(faces).reshape(-1, 3)):
        terms = face_terms(cam, len(cam), tri)
        if terms is None:
            continue
        nA, nB, nC, det, A, B, C = terms
        if A[2] < near and B[2] < near and C[2] < near:
            continue      # the face takes no part
        with np.errstate(all="ignore"):
            w = [(rx * n[0] + ry * n[1]) + n[2] for n in (nA, nB, nC)]
            s = (w[0] + w[1]) + w[2]
            inside = (w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0) if det > 0 else (w[0] <= 0) & (w[1] <= 0) & (w[2] <= 0)
            z = det / s
            better = inside & (s != 0) & np.isfinite(z) & (z >= near) & (z < depth)
            low = np.minimum(np.minimum(w[0] / s, w[1] / s), w[2] / s)
        depth, face, margin = np.where(better, z, depth), np.where(better, f, face).astype(np.int32), np.where(better, low, margin)
    return np.where(face >= 0, depth, 0.0), face, margin


# ---- virtual views ------------------------------------------------------------------------------------------------------------------------
def splitmix(seed, n):
    mask = 2 ** 64 - 1
    z = (seed + n * 0x9E3779B97F4A7C15) & mask
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
    return z ^ (z >> 31)


def view_choice(T, M, i, seed=0):
    """(the pose, the target) view i takes"""
    return splitmix(seed, 3 * i + 1) % T, splitmix(seed, 3 * i + 2) % M


def view_case(w2cs, targets, i, seed=0):
    """"pose" (the target sits at the centre), "fallback" (the viewing direction is within 1e-3 of the pose's image-down axis) or
    "down", for view i"""
    w2cs, targets = np.asarray(w2cs, np.float64), np.asarray(targets, np.float64)
    a, b = view_choice(len(w2cs), len(targets), i, seed)
    R, t = w2cs[a][:3, :3], w2cs[a][:3, 3]
    d = targets[b] - (-R.T @ t)
    if np.linalg.norm(d) < 1e-6:
        return "pose"
    return "fallback" if np.linalg.norm(np.cross(d / np.linalg.norm(d), R[1])) < 1e-3 else "down"


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------
PLANE_K = np.array([[40.0, 0, 31.5], [0, 40.0, 23.5], [0, 0, 1]])
PLANE_H, PLANE_W = 48, 64


def tilted_plane(seed=0, n=9):
    """(vertices float32 [81,3], faces int32 [128,3]) of the plane z = 3 + 0.4 x - 0.3 y over a jittered 9 x 9 grid on [-4, 4]^2, in
    camera coordinates (render it with the identity): every triangle with a random winding and a random rotation of its corners"""
    rng = np.random.default_rng(seed)
    g = np.linspace(-4, 4, n)
    X, Y = np.meshgrid(g, g)
    X = X + rng.uniform(-0.3, 0.3, X.shape)
    Y = Y + rng.uniform(-0.3, 0.3, Y.shape)
    vertices = np.stack([X, Y, 3 + 0.4 * X - 0.3 * Y], -1).reshape(-1, 3).astype(F32)
    faces = []
    for j in range(n - 1):
        for i in range(n - 1):
            a = j * n + i
            b, c, d = a + 1, a + n, a + n + 1
            for t in ([a, b, c], [b, d, c]):
                if rng.random() < 0.5:
                    t = [t[0], t[2], t[1]]
                r = int(rng.integers(3))
                faces.append(t[r:] + t[:r])
    return vertices, np.array(faces, np.int32)


def place(vertices, w2c):
    """camera-space vertices -> float32 world-space vertices that w2c maps back to them (to rounding): the scene placed with the inverse
    camera, so that it stays in view whatever the camera"""
    m = np.asarray(w2c, np.float64)
    return ((np.asarray(vertices, np.float64) - m[:3, 3]) @ m[:3, :3]).astype(F32)


def random_faces(seed, k, H, W, n=160):
    """(vertices float32 [3n,3], faces int32 [n,3]) in camera coordinates: n triangles at depths of 0.6 to 4 around pixel centres spread over
    the image and a margin around it, from a pixel or two across to a third of the image, both windings; two have one corner pushed
    behind the camera"""
    rng = np.random.default_rng(seed)
    k = np.asarray(k, np.float64)
    vertices, faces = [], []
    for i in range(n):
        u, v, z = rng.uniform(-6, W + 6), rng.uniform(-6, H + 6), rng.uniform(0.6, 4.0)
        size = float(rng.choice([1.2, 3.0, 8.0, W / 3.0]))
        tri = []
        for j in range(3):
            du, dv = rng.uniform(-size, size, 2)
            zz = z + rng.uniform(-0.3, 0.3)
            if i in (57, 121) and j == 2:
                zz = -0.4
            tri.append([(u + du - k[0][2]) / k[0][0] * zz, (v + dv - k[1][2]) / k[1][1] * zz, zz])
        vertices += tri
        faces.append([3 * i, 3 * i + 1, 3 * i + 2] if rng.random() < 0.5 else [3 * i, 3 * i + 2, 3 * i + 1])
    return np.array(vertices, F32), np.array(faces, np.int32)


def plane_truth():
    """(t float64 [H,W], inner bool [H,W]): the depth at which the ray of every pixel centre of the plane scene meets the analytic
    plane, and whether that point lies within |x|, |y| < 3.6: inside the mesh whatever the jitter of its border (at most 0.3 from 4)"""
    rx = ((np.arange(PLANE_W) - PLANE_K[0][2]) / PLANE_K[0][0])[None, :]
    ry = ((np.arange(PLANE_H) - PLANE_K[1][2]) / PLANE_K[1][1])[:, None]
    t = 3 / (1 - 0.4 * rx + 0.3 * ry)
    return t, (np.abs(t * rx) < 3.6) & (np.abs(t * ry) < 3.6) & (t > 0)


def box_room(half=(2.0, 1.5, 3.0), far=None):
    """(vertices float32 [8,3], faces int32 [12,3]) of a box room around the origin with the given half sizes; far: the z of its far
    wall (the wall at +half[2]) when it is moved"""
    hx, hy, hz = half
    zf = hz if far is None else far
    v = np.array([[-hx, -hy, -hz], [hx, -hy, -hz], [hx, hy, -hz], [-hx, hy, -hz], [-hx, -hy, zf], [hx, -hy, zf], [hx, hy, zf], [-hx, hy, zf]], F32)
    quads = [(0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (3, 2, 6, 7), (0, 3, 7, 4), (1, 2, 6, 5)]
    f = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return v, np.array(f, np.int32)
