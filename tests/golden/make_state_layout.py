"""Records tests/golden/state_layout.json: the sizes of the three state buffers and every field of hsr_get_state_layout over the grid
below, from the library HSR_RAST_LIB names (default: the tree's).  The committed file was recorded from the build of the commit BEFORE
the layouts moved into csrc/hsr_state.hip; tests/test_state_layout_cpu.py holds every later build to it exactly.  Host arithmetic only:
needs no GPU.  Run: HSR_RAST_LIB=<parent build>/libhsr_rast.so python tests/golden/make_state_layout.py"""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "hier-slam_amd"))

GRID_P = [0, 1, 255, 256, 257, 1000, 500000]
GRID_WH = [(1, 1), (16, 16), (17, 31), (64, 48), (1200, 680), (1920, 1080)]
GRID_R = [0, 1, 4095, 4096, 4097, 5000, 3000000, 2147483647]


def record(_C):
    lib = _C._lib
    fields = [n for n, _ in _C._StateLayout._fields_]
    return {
        "P": GRID_P, "WH": [list(wh) for wh in GRID_WH], "R": GRID_R, "fields": fields,
        "geometry_bytes": [lib.hsr_required_geometry_bytes(P) for P in GRID_P],
        "image_bytes": [lib.hsr_required_image_bytes(W, H) for W, H in GRID_WH],
        "binning_bytes": [lib.hsr_required_binning_bytes(R) for R in GRID_R],
        # one row per (P, (W, H), R) of itertools.product(P, WH, R), the fields in the order of "fields"
        "layout": [[_C.state_layout(P, W, H, R)[n] for n in fields] for P, (W, H), R in itertools.product(GRID_P, GRID_WH, GRID_R)],
    }


if __name__ == "__main__":
    from diff_gaussian_rasterization import _C
    with open(os.path.join(HERE, "state_layout.json"), "w") as f:
        json.dump(record(_C), f, separators=(",", ":"))
        f.write("\n")
    print("recorded from", _C._LIB_PATH)
