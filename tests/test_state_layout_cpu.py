"""CPU suite: the sizes of the three state buffers and every offset hsr_get_state_layout reports equal, byte for byte, what the library
computed before the layouts were restated as integer offsets in csrc/hsr_state.hip (tests/golden/state_layout.json, recorded from that
earlier build by tests/golden/make_state_layout.py).  Host arithmetic only: there is no GPU here."""
import itertools
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "state_layout.json")
GRID_P = [0, 1, 255, 256, 257, 1000, 500000]
GRID_WH = [(1, 1), (16, 16), (17, 31), (64, 48), (1200, 680), (1920, 1080)]
GRID_R = [0, 1, 4095, 4096, 4097, 5000, 3000000, 2147483647]


def _golden():
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert gold["P"] == GRID_P and [tuple(wh) for wh in gold["WH"]] == GRID_WH and gold["R"] == GRID_R
    return gold


def test_required_bytes_equal_recorded():
    from diff_gaussian_rasterization import _C
    lib, gold = _C._lib, _golden()
    assert [lib.hsr_required_geometry_bytes(P) for P in GRID_P] == gold["geometry_bytes"]
    assert [lib.hsr_required_image_bytes(W, H) for W, H in GRID_WH] == gold["image_bytes"]
    assert [lib.hsr_required_binning_bytes(R) for R in GRID_R] == gold["binning_bytes"]
    # values measured on the earlier build, stated independently of the file
    assert lib.hsr_required_geometry_bytes(1000) == 144640
    assert lib.hsr_required_image_bytes(64, 48) == 37376
    assert lib.hsr_required_binning_bytes(5000) == 124160


def test_state_layout_equals_recorded():
    from diff_gaussian_rasterization import _C
    gold = _golden()
    fields = [n for n, _ in _C._StateLayout._fields_]
    assert fields == gold["fields"] and len(fields) == 17
    cases = list(itertools.product(GRID_P, GRID_WH, GRID_R))
    assert len(cases) == len(gold["layout"]) == 336
    for (P, (W, H), R), want in zip(cases, gold["layout"]):
        lay = _C.state_layout(P, W, H, R)
        assert [lay[n] for n in fields] == want, (P, W, H, R)
    lay = _C.state_layout(1000, 64, 48, 5000)
    assert lay["img_final_T"] == 256 and lay["bin_vals"] == 100608
