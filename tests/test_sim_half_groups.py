"""CPU: tests/sim_half_groups.py (the trip count behind EXPERIMENTS.md §10o) against tests/sim_line0_rows.py on a small scene — both re-evaluate
hsr_tile_common.h's subblock_mask in numpy, each in its own words, and must agree on every row count they share — and the properties the
half-block rule has to have whatever the scene."""
import os
import re
import subprocess
import sys

import pytest

import sim_half_groups as S

HERE = os.path.dirname(os.path.abspath(__file__))
P, BATCH = 20000, 224


@pytest.fixture(scope="module")
def counts():
    return S.count(S.load(P, "slam"), BATCH)


def test_row_counts_equal_sim_line0_rows(counts):
    out = subprocess.run([sys.executable, os.path.join(HERE, "sim_line0_rows.py"), str(P), "slam", str(BATCH), "3"], check=True,
                         capture_output=True, text=True).stdout

    def figure(label):
        m = re.search(re.escape(label) + r"\s+(\d+)", out)
        assert m, (label, out)
        return int(m.group(1))

    assert figure("list instances (num_rendered)") == counts["instances"]
    assert figure("of which reach no sub-block of their tile") == counts["reach_none"]
    assert figure("(instance, quadrant) rows the kernel sends") == counts["rows_q"]
    assert figure("rows if sent once per (instance, tile)") == counts["rows_t"]


def test_half_rule(counts):
    assert counts["instances"] > 10000 and counts["reach_none"] > 0
    assert counts["half_misses"] == 0                       # no half with an accepting pixel is dropped
    assert counts["slab"]["4x4"][0] == counts["sub_entries"]  # the folded 4x4 lists are subblock_mask's bits
    for rule in ("pixel", "slab"):
        v4, t4, s4 = counts[rule]["4x4"]
        v2, t2, s2 = counts[rule]["4x2"]
        assert v4 <= v2 <= 2 * v4 and t2 <= t4 and s2 <= s4   # twice the lists, each no longer than the sub-block's
    for n in ("4x4", "4x2"):                                 # the kernel's lists hold every group the pixel rule lists
        assert counts["pixel"][n][0] <= counts["slab"][n][0] and counts["pixel"][n][1] <= counts["slab"][n][1] + 1e-9
