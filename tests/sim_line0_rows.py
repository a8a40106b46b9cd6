#!/usr/bin/env python3
"""Not a test: the CPU count behind EXPERIMENTS.md §10h "line 0 of a gradient row once per (splat, tile)".  Takes the sorted instance list,
the geometry state and the per-pixel contributor counts of a headline-sized scene from the oracle, re-evaluates hsr_tile_common.h's
subblock_mask (as tests/sim_sublists.py does) and each pixel's accept test in numpy, walks every tile's list in the backward tile kernel's
batches (a quadrant's wave skips a batch that lies wholly behind its last contributor) and prints
  * the list instances, and how many of them reach no sub-block of their tile;
  * the (instance, quadrant) gradient rows the kernel sends — one request per 64-byte line each — and how many of them carry a value
    (some pixel of the quadrant accepts the splat: a row of zeros keeps its line 0 at home, hsr_render_bwd_q.hip);
  * the rows if one were sent per (instance, tile), and how many of those carry a value;
  * the memory-side atomic requests per launch that follow for rows of `lines` 64-byte lines, with line 0 per quadrant and per tile.
Usage: python tests/sim_line0_rows.py [P] [slam|aniso] [batch] [lines]   (default 500000 slam 224 3: the K = 26 headline; ~20 s, ~3 GB)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "hier-slam_amd")]
import oracle_lib as O  # noqa: E402
from hsr_utils.camera import replica_intrinsics, setup_camera_tensors  # noqa: E402
from hsr_utils.synthetic import make_scene  # noqa: E402

W, H, K = 1200, 680, 4   # the lists, the masks and the accept tests do not depend on K
P = int(sys.argv[1]) if len(sys.argv) > 1 else 500000
kind = sys.argv[2] if len(sys.argv) > 2 else "slam"
BATCH = int(sys.argv[3]) if len(sys.argv) > 3 else 224
LINES = int(sys.argv[4]) if len(sys.argv) > 4 else 3
k = replica_intrinsics(W, H)
cam = setup_camera_tensors(W, H, k, np.eye(4))
sc = make_scene(P, W, H, K, k, seed=0, kind=kind)
_, st = O.forward(cam, sc["means3D"], sc["opacities"], colors_precomp=sc["colors_precomp"], semantics_precomp=sc["semantics_precomp"],
                  scales=sc["scales"], rotations=sc["rotations"])
m2, co = st.field("means2D"), st.field("conic_opacity")
keys, vals = st.field("keys"), st.field("vals")
ranges = np.asarray(st.field("ranges")).reshape(-1, 2).astype(np.int64)
n_contrib = np.asarray(st.field("n_contrib")).reshape(H, W).astype(np.int64)
tiles = (keys >> np.uint64(32)).astype(np.int64)
g = vals.astype(np.int64)
R = len(g)
tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
f = np.float32
tx, ty = ((tiles % tiles_x) * 16).astype(f), ((tiles // tiles_x) * 16).astype(f)
x, y = m2[g, 0].astype(f), m2[g, 1].astype(f)
A, B, C, o = [co[g, i].astype(f) for i in range(4)]

# ---- which quadrants of its tile an instance reaches: subblock_mask (exact row-slab test), folded to the four 8x8 quadrants ----
t255 = f(255) * o
ok = t255 >= 1
tau = f(2) * np.log(np.maximum(t255, 1)).astype(f) * f(1.002) + f(0.02)
det = A * C - B * B
inv_a = f(1) / A
hy = np.sqrt(tau * A * (f(1) / det)) * f(1.001) + f(0.02)
dyp, atau, nb = -(B / C) * np.sqrt(tau * C * (f(1) / det)), A * tau, -B
rx, ry = x - tx, y - ty
quad = np.zeros((R, 4), bool)   # [instance][2 * (lower half) + (right half)]
for r in range(4):
    lo, hi = np.maximum(ry - f(4 * r + 3), -hy), np.minimum(ry - f(4 * r), hy)
    top = np.maximum(lo, hi)
    dyu, dyl = np.clip(dyp, lo, top), np.clip(-dyp, lo, top)
    xmax = (nb * dyu + np.sqrt(np.maximum(atau - det * dyu * dyu, 0))) * inv_a + f(0.02)
    xmin = (nb * dyl - np.sqrt(np.maximum(atau - det * dyl * dyl, 0))) * inv_a - f(0.02)
    row_on = (lo <= hi) & ok
    for c in range(4):
        quad[:, 2 * (r >> 1) + (c >> 1)] |= row_on & ((rx - f(4 * c + 3)) <= xmax) & ((rx - f(4 * c)) >= xmin)

# ---- the kernel's walk: position of an instance in its tile's list, the tile's and each quadrant's last contributor, batches from the back ----
pos = np.arange(R, dtype=np.int64) - ranges[tiles, 0]
nc = np.zeros((tiles_y * 16, tiles_x * 16), np.int64)
nc[:H, :W] = n_contrib
ncq = nc.reshape(tiles_y, 2, 8, tiles_x, 2, 8).max(axis=(2, 5)).transpose(0, 2, 1, 3).reshape(tiles_y * tiles_x, 4)   # [tile][quadrant]
hi_all = ncq.max(axis=1)
staged = pos < hi_all[tiles]
batch_lo = hi_all[tiles] - ((hi_all[tiles] - 1 - pos) // BATCH + 1) * BATCH   # first position of the instance's batch (may be negative)
visits = staged[:, None] & quad & (np.maximum(batch_lo, 0)[:, None] < ncq[tiles])   # the quadrant's wave does not skip the batch

# ---- does some pixel of the quadrant accept the splat?  (the forward's test: power <= 0, alpha >= 1/255, in front of the pixel's last contributor) ----
carries = np.zeros((R, 4), bool)
py_, px_ = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
qof = (2 * (py_ >> 3) + (px_ >> 3)).reshape(-1)
nct = nc.reshape(tiles_y, 16, tiles_x, 16).transpose(0, 2, 1, 3).reshape(tiles_y * tiles_x, 256)
for s in range(0, R, 65536):
    e = slice(s, min(s + 65536, R))
    dx = x[e, None] - (tx[e, None] + px_.reshape(-1).astype(f)[None])
    dy = y[e, None] - (ty[e, None] + py_.reshape(-1).astype(f)[None])
    power = f(-0.5) * (A[e, None] * dx * dx + C[e, None] * dy * dy) - B[e, None] * dx * dy
    alpha = np.minimum(f(0.99), o[e, None] * np.exp(np.minimum(power, 0)))
    acc = (power <= 0) & (alpha >= f(1.0 / 255.0)) & (pos[e, None] < nct[tiles[e]])
    for q in range(4):
        carries[e, q] = acc[:, qof == q].any(axis=1)
carries &= visits

rows_q, rows_q_val = int(visits.sum()), int(carries.sum())
rows_t, rows_t_val = int(visits.any(axis=1).sum()), int(carries.any(axis=1).sum())
reach = quad.any(axis=1)
print("%s scene, P = %d, batches of %d, rows of %d lines" % (kind, P, BATCH, LINES))
print("list instances (num_rendered)                                   %9d" % R)
print("  of which reach no sub-block of their tile                     %9d (%.1f %%)" % (int((~reach).sum()), 100.0 * (~reach).mean()))
print("  of which reach one / two / three / four quadrants             %s" % " / ".join("%d" % int((quad.sum(axis=1) == n).sum()) for n in (1, 2, 3, 4)))
print("(instance, quadrant) rows the kernel sends                      %9d" % rows_q)
print("  of which some pixel accepts the splat                         %9d (%.1f %%)" % (rows_q_val, 100.0 * rows_q_val / max(rows_q, 1)))
print("rows if sent once per (instance, tile)                          %9d (%.2f quadrants per row)" % (rows_t, rows_q / max(rows_t, 1)))
print("  of which some pixel accepts the splat                         %9d" % rows_t_val)
now, merged = (LINES - 1) * rows_q + rows_q_val, (LINES - 1) * rows_q + rows_t_val
print("atomic requests per launch, line 0 per quadrant                 %9d" % now)
print("atomic requests per launch, line 0 per tile                     %9d (%+.1f %%; line 0 alone %+.1f %%)" % (
    merged, 100.0 * (merged - now) / max(now, 1), 100.0 * (rows_t_val - rows_q_val) / max(rows_q_val, 1)))
st.free()
