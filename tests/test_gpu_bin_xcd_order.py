"""-m gpu: the tile binning's count table summed in XCD-major row order (hsr_common.h: hsr_bin_row_of; bin_scan_kernel, bin_emit_kernel in
hsr_preprocess.hip), against the oracle: num_rendered, point_offsets, sorted keys, values and tile ranges bit for bit, and the images and
gradients of one forward + backward at the harness's usual bounds.

bin_scan_kernel takes the exclusive prefix over the nblk rows of table[nblk][T] in the order "rows with b mod 8 = 0 ascending, then 1,
... 7" (row b = workgroup b of bin_hist / bin_emit = one 1 024-Gaussian chunk here), so that the part of a tile segment that one XCD's
L2 writes is contiguous.  Any bijection gives the same sorted lists; a map that is none gives overlapping or torn segments, which the
keys and values show at once.

Cases: a 160 x 96 image (T = 60 tiles) with P chosen so that nblk = ceil(P / 1024) is 1, 3 and 7 (nblk < 8: the identity), 8 and 16
(no remainder), 9 and 17 (remainder 1), 15 and 23 (remainder 7), 10 (one row per class and two classes with a second row); one case at
64 x 64 (T = 16: the smallest table, one workgroup of bin_scan_kernel, most of it past T); and two variants of nblk = 17: every Gaussian
of the rows with b mod 8 = 3 behind the camera (a class without a single instance), and only the rows of class 5 in front of it (every
segment is one sub-segment).  Scene: hsr_utils.synthetic's "slam" kind at scale_mult 2.5: rects of 1 x 1 up to 3 x 3 tiles and more
(checked below on the oracle's tiles_touched).  Seeds: the oracle flags no tie-risk pixel for any of them (checked below), so the
comparison of the images and gradients needs no tie bound.

Every case runs the plain forward (with its backward), the second forward of the same size (emit, sort and render enqueued before the
count is read back: the speculative launch) and the forward that finds a binning buffer too small (the fall-back: the same kernels
again with plain pointers), set up as tests/test_gpu_tile_sort_edges.py does."""
import numpy as np
import pytest
import torch

import harness
import scenes
from harness import run_gpu, run_oracle
from test_gpu_parity import _compare_integers

pytestmark = pytest.mark.gpu

K = 3
SCALE_MULT = 2.5
CHUNK = 1024   # Gaussians per binning workgroup for P <= 2^18 (hsr_bin_plan)

# name: (W, H, nblk, variant, seed)
CASES = {
    "nblk1": (160, 96, 1, None, 3),
    "nblk3": (160, 96, 3, None, 4),
    "nblk7": (160, 96, 7, None, 152),
    "nblk8": (160, 96, 8, None, 133),
    "nblk9": (160, 96, 9, None, 312),
    "nblk10": (160, 96, 10, None, 172),
    "nblk15": (160, 96, 15, None, 264),
    "nblk16": (160, 96, 16, None, 50),
    "nblk17": (160, 96, 17, None, 238),
    "nblk23": (160, 96, 23, None, 601),
    "tiny_table_64x64": (64, 64, 9, None, 3),
    "nblk17_class3_behind": (160, 96, 17, "class3_behind", 641),
    "nblk17_only_class5": (160, 96, 17, "only_class5", 3),
}


def _scene(name):
    W, H, nblk, variant, seed = CASES[name]
    P = CHUNK * (nblk - 1) + 411                          # the last chunk is ragged
    cam, sc, up = scenes.build(W, H, P, K, seed=seed, kind="slam", scale_mult=SCALE_MULT, tilt=False)
    if variant:
        row = torch.arange(P) // CHUNK
        behind = (row % 8 == 3) if variant == "class3_behind" else (row % 8 != 5)
        sc["means3D"][behind, 2] = -1.0
    return cam, sc, up


class _Oracle:
    """one oracle run (forward + backward) per case, shared by its three tests; states freed at the end of the module"""

    def __init__(self):
        self.runs = {}

    def get(self, name, cam, sc, up):
        if name not in self.runs:
            self.runs[name] = run_oracle(cam, sc, up, semantic=True)
        return self.runs[name]

    def close(self):
        for _, _, st in self.runs.values():
            st.free()
        self.runs.clear()


@pytest.fixture(scope="module")
def oracle():
    o = _Oracle()
    yield o
    o.close()


def _hint_key(sc, W, H):
    return (torch.device("cuda:0").index or 0, int(sc["means3D"].shape[0]), W, H)


def check_scene(name, sc, out_o, st_o):
    """the scene is what the docstring says it is (also run on the CPU when the case list was chosen)"""
    W, H, nblk, variant, _ = CASES[name]
    P = sc["means3D"].shape[0]
    assert (P + CHUNK - 1) // CHUNK == nblk and P <= 1 << 18
    touched = st_o.field("tiles_touched")
    assert int(touched[touched > 0].min()) == 1 and int(touched.max()) >= 9, (int(touched.min()), int(touched.max()))
    assert out_o["num_rendered"] > 1024     # larger than the buffer a hint of 0 gives: the fall-back test takes the fall-back
    assert int(st_o.field("tie_pixels").astype(bool).sum()) == 0
    assert st_o.bounds_info["overflow_pixels"] == 0, st_o.bounds_info
    row = np.arange(P) // CHUNK
    per_row = np.bincount(row, weights=touched, minlength=nblk)
    if variant == "class3_behind":
        assert (per_row[row_classes(nblk) == 3] == 0).all() and (per_row[row_classes(nblk) != 3] > 0).all()
    elif variant == "only_class5":
        assert (per_row[row_classes(nblk) != 5] == 0).all() and (per_row[row_classes(nblk) == 5] > 0).all()
    else:
        assert (per_row > 0).all()


def row_classes(nblk):
    return np.arange(nblk) % 8


@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_backward(oracle, name):
    from diff_gaussian_rasterization import _C
    W, H = CASES[name][:2]
    cam, sc, up = _scene(name)
    out_o, gr_o, st_o = oracle.get(name, cam, sc, up)
    check_scene(name, sc, out_o, st_o)
    _C._binning_hint.pop(_hint_key(sc, W, H), None)
    out_g, gr_g, st_g = run_gpu(cam, sc, up, semantic=True)
    _compare_integers(out_g, st_g, out_o, st_o)
    for n in ("color", "depth", "opacity", "semantic"):
        harness.assert_close(n, out_g[n], out_o[n], allowance=harness.tie_allowance(n, st_o, out_g[n].shape, "pixel"))
    for n in gr_o:
        harness.assert_close("grad " + n, gr_g[n], gr_o[n], allowance=harness.tie_allowance("grad " + n, st_o, gr_g[n].shape, "gauss"))


@pytest.mark.parametrize("name", list(CASES))
def test_second_forward_of_the_same_size(oracle, name):
    from diff_gaussian_rasterization import _C
    W, H = CASES[name][:2]
    cam, sc, up = _scene(name)
    out_o, _, st_o = oracle.get(name, cam, sc, up)
    key = _hint_key(sc, W, H)
    _C._binning_hint.pop(key, None)
    for _ in range(2):
        out_g, _, st_g = run_gpu(cam, sc, up, semantic=True)
        _compare_integers(out_g, st_g, out_o, st_o)
        assert _C._binning_hint[key] == out_o["num_rendered"]


@pytest.mark.parametrize("name", list(CASES))
def test_binning_buffer_too_small(oracle, name):
    from diff_gaussian_rasterization import _C
    W, H = CASES[name][:2]
    cam, sc, up = _scene(name)
    out_o, _, st_o = oracle.get(name, cam, sc, up)
    key = _hint_key(sc, W, H)
    _C._binning_hint[key] = 0
    out_g, _, st_g = run_gpu(cam, sc, up, semantic=True)
    _compare_integers(out_g, st_g, out_o, st_o)
    assert _C._binning_hint[key] == out_o["num_rendered"] > 1024
