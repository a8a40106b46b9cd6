"""-m gpu: the per-tile sort and the instance emission at the edges of their code paths (hsr_sort.hip, hsr_sort_net.h, bin_emit_kernel),
keys, values and tile ranges bit for bit against the oracle.

Scene of the length tests: a 32 x 16 image = two tiles, n splats of ~43 pixels radius around the middle, so that BOTH tiles hold exactly
n entries and the second tile's segment starts at entry n (odd n: a segment that does not start on 16 bytes).  Every opacity is 0.002,
so no alpha reaches 1/255, nothing contributes, and no pixel takes a decision near a threshold (the oracle's tie_pixels is checked to be
empty): the comparison is about the lists alone.

Lengths: each register network's first, last and one-past sizes (two waves with 2, 4 and 8 composites per lane: <= 256, <= 512,
<= 1 024; four waves with 8: <= 2 048; the block radix sort beyond), where the 16-byte loads and stores of a lane's run give way to the
element-wise ragged end, plus 1, 2 and 3.  Depth patterns: ascending with the index, descending, random, and all equal with the
Gaussians numbered at random (the index half of the composite alone decides).

The emission test spans rects of 1x1, 1x5, 5x1, 3x3 and 7x7 tiles on 112 x 112 (1, 5, 5, 9 and 49 instances per splat) and 2x2, 2x3 and
3x5 (4, 6, 15), the shapes interleaved so that neighbouring lanes of bin_emit_kernel walk rects of different sizes, some of them centred
outside the image.  It was written for an emission that takes the cursors of four tiles per wait (every remainder of a batch of four is
there); that emission measured no faster and was not kept (EXPERIMENTS §10l), the test holds for any order of the cursors."""
import numpy as np
import pytest
import torch

from harness import run_gpu, run_oracle
from hsr_utils.camera import replica_intrinsics, setup_camera_tensors
from hsr_utils.synthetic import make_upstream_grads
from test_gpu_parity import _compare_integers

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049]
PATTERNS = ("ascending", "descending", "random", "equal_shuffled")
W, H, K = 32, 16, 3


def _splats(W, H, px, py, z, radius_px, seed):
    """isotropic Gaussians whose centres project to (px, py) at depth z and whose LARGER screen-space sigma is radius_px / 3"""
    k = replica_intrinsics(W, H)
    fx, fy, cx, cy = k[0][0], k[1][1], k[0][2], k[1][2]
    P = z.shape[0]
    means = torch.stack([((px - cx) / fx) * z, ((py - cy) / fy) * z, z], 1)
    s = (radius_px / 3.0) * z / max(fx, fy)
    rots = torch.zeros(P, 4)
    rots[:, 0] = 1
    g = torch.Generator(device="cpu").manual_seed(seed)
    sc = dict(means3D=means, scales=s[:, None].repeat(1, 3), rotations=rots, opacities=torch.full((P, 1), 0.002),
              colors_precomp=torch.rand(P, 3, generator=g), semantics_precomp=torch.rand(P, K, generator=g))
    return {n: v.float().contiguous() for n, v in sc.items()}


def _camera(W, H):
    cam = setup_camera_tensors(W, H, replica_intrinsics(W, H), np.eye(4))
    cam["bg"] = torch.zeros(3, dtype=torch.float32)
    up = {n: v * float(W * H) for n, v in make_upstream_grads(W, H, K, seed=1).items()}
    return cam, up


def _two_tile_scene(n, pattern, culled=False):
    g = torch.Generator(device="cpu").manual_seed(1000 * n + PATTERNS.index(pattern))
    # centres off the pixel grid, 10..22 x 4..12: with a radius of ~43 pixels every rect is the whole image
    px = 10.37 + 12.0 * torch.rand(n, generator=g)
    py = 4.41 + 8.0 * torch.rand(n, generator=g)
    i = torch.arange(n, dtype=torch.float32)
    if pattern == "ascending":
        z = 2.0 + 1e-3 * i
    elif pattern == "descending":
        z = 2.0 + 1e-3 * (n - 1 - i)
    elif pattern == "random":
        z = 2.0 + 2.0 * torch.rand(n, generator=g)
    else:
        z = torch.full((n,), 2.5)
    sc = _splats(W, H, px, py, z, 42.0, seed=n)
    if culled:
        # a Gaussian behind the camera (radius 0) in front of every tenth one: the indices in the lists are no longer consecutive
        order = []
        for j in range(n):
            if j % 10 == 0:
                order.append(-1)
            order.append(j)
        idx = torch.tensor([max(o, 0) for o in order])
        behind = torch.tensor([o < 0 for o in order])
        sc = {m: v[idx].clone() for m, v in sc.items()}
        sc["means3D"][behind, 2] = -1.0
    cam, up = _camera(W, H)
    return cam, sc, up


class _Oracle:
    """one oracle run per scene, shared by the tests that look at the same scene; states freed at the end of the module"""

    def __init__(self):
        self.runs = {}

    def get(self, key, cam, sc, up):
        if key not in self.runs:
            out_o, _, st_o = run_oracle(cam, sc, up, semantic=True)
            self.runs[key] = (out_o, st_o)
        return self.runs[key]

    def close(self):
        for _, st in self.runs.values():
            st.free()
        self.runs.clear()


@pytest.fixture(scope="module")
def oracle():
    o = _Oracle()
    yield o
    o.close()


def _hint_key(sc, w, h):
    return (torch.device("cuda:0").index or 0, int(sc["means3D"].shape[0]), w, h)


def _check(oracle, key, cam, sc, up, n, entries_per_tile=None):
    out_o, st_o = oracle.get(key, cam, sc, up)
    out_g, _, st_g = run_gpu(cam, sc, up, semantic=True)
    if entries_per_tile is not None:
        ranges = st_o.field("ranges")
        assert [int(b - a) for a, b in ranges] == [entries_per_tile] * len(ranges), ranges   # the scene is what the test says it is
        assert int(st_o.field("tie_pixels").astype(bool).sum()) == 0
    _compare_integers(out_g, st_g, out_o, st_o)
    return st_g


@pytest.mark.parametrize("n", LENGTHS)
def test_list_lengths(oracle, n):
    from diff_gaussian_rasterization import _C
    for pattern in PATTERNS:
        cam, sc, up = _two_tile_scene(n, pattern)
        _C._binning_hint.pop(_hint_key(sc, W, H), None)
        _check(oracle, (n, pattern, False), cam, sc, up, n, entries_per_tile=n)


@pytest.mark.parametrize("n", LENGTHS)
def test_culled_gaussians_in_front(oracle, n):
    cam, sc, up = _two_tile_scene(n, "random", culled=True)
    assert sc["means3D"].shape[0] == n + (n + 9) // 10
    st_g = _check(oracle, (n, "random", True), cam, sc, up, n, entries_per_tile=n)
    assert st_g["num_rendered"] == 2 * n


@pytest.mark.parametrize("n", LENGTHS)
def test_second_forward_of_the_same_size(oracle, n):
    """the second forward of a (P, W, H) finds a binning buffer sized from the first one's count: emit, sort and render are enqueued
    before the count is read back and resolve their arrays on the device (the speculative launch)"""
    from diff_gaussian_rasterization import _C
    cam, sc, up = _two_tile_scene(n, "random")
    key = _hint_key(sc, W, H)
    _C._binning_hint.pop(key, None)
    _check(oracle, (n, "random", False), cam, sc, up, n)
    assert _C._binning_hint[key] == 2 * n
    _check(oracle, (n, "random", False), cam, sc, up, n)
    assert _C._binning_hint[key] == 2 * n


@pytest.mark.parametrize("n", LENGTHS)
def test_binning_buffer_too_small(oracle, n):
    """a hint of 0 gives a buffer for 1 024 instances: from 513 entries per tile on the speculative kernels find it too small and return,
    and the forward grows it and runs emit, sort and render again with the arrays handed over as plain pointers (the fall-back)"""
    from diff_gaussian_rasterization import _C
    cam, sc, up = _two_tile_scene(n, "descending")
    key = _hint_key(sc, W, H)
    _C._binning_hint[key] = 0
    _check(oracle, (n, "descending", False), cam, sc, up, n)
    assert _C._binning_hint[key] == 2 * n


# name: (centre x, centre y, radius in pixels, columns, rows) on 112 x 112 = 7 x 7 tiles; centres may lie outside the image
RECTS = {
    "1x1": (56.3, 56.3, 4.0, 1, 1),
    "1x5": (-30.3, 56.3, 35.0, 1, 5),
    "5x1": (56.3, -30.3, 28.0, 5, 1),     # above the image the projection's clamp widens the footprint by a quarter: 36 pixels again
    "3x3": (56.3, 56.3, 19.0, 3, 3),
    "7x7": (56.3, 56.3, 90.0, 7, 7),
    "2x2": (64.3, 64.3, 4.0, 2, 2),
    "2x3": (64.3, 56.3, 11.0, 2, 3),
    "3x5": (8.3, 56.3, 35.0, 3, 5),
}
EMIT_COPIES = 40


def _rect_scene():
    WE = HE = 112
    names = list(RECTS) * EMIT_COPIES                     # the shapes interleaved: neighbouring lanes hold rects of different sizes
    g = torch.Generator(device="cpu").manual_seed(11)
    jit = 0.4 * (torch.rand(len(names), 2, generator=g) - 0.5)
    px = torch.tensor([RECTS[m][0] for m in names]) + jit[:, 0]
    py = torch.tensor([RECTS[m][1] for m in names]) + jit[:, 1]
    r = torch.tensor([RECTS[m][2] for m in names])
    z = 2.0 + 2.0 * torch.rand(len(names), generator=g)
    sc = _splats(WE, HE, px, py, z, r, seed=12)
    cam, up = _camera(WE, HE)
    return cam, sc, up, names


def test_emit_rect_shapes(oracle):
    cam, sc, up, names = _rect_scene()
    out_o, st_o = oracle.get("rects", cam, sc, up)
    want = np.array([RECTS[m][3] * RECTS[m][4] for m in names], dtype=np.uint32)
    assert np.array_equal(st_o.field("tiles_touched"), want), sorted(set(zip(names, st_o.field("tiles_touched").tolist())))
    _check(oracle, "rects", cam, sc, up, 0)
    _check(oracle, "rects", cam, sc, up, 0)    # and through the second forward of this size
