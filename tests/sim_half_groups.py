#!/usr/bin/env python3
"""Not a test: the CPU count behind EXPERIMENTS.md §10o "eight-lane groups on 4x2 half-blocks in the forward's visit loop".  Takes the
sorted instance list and the geometry state of a headline-sized scene from the oracle and counts, for lane groups of 4x4 (sixteen lanes,
four lists per wave), 4x2 and 2x4 (eight lanes, eight lists) and 2x2 pixels (four lanes, sixteen lists), with every list taken whole:
  * the group visits: the sum of the lengths of all groups' lists;
  * the trips of a wave's visit loop per tile, i.e. the longest of the wave's lists, averaged over tiles and waves;
  * the same for the slowest of a tile's four waves.
Two visit rules are counted.  "pixel": a group lists a splat iff the splat's alpha >= 1/255 region holds the centre of one of the group's
pixels (the best any rule can do).  "slab": hsr_tile_common.h's rules re-evaluated in numpy — subblock_mask for 4x4 (as tests/sim_sublists.py
does) and subblock_half_mask for 4x2: a half of a 4x4 block whose bit is set is listed iff its two pixel rows meet the region's extent
in y; these are the lists the kernel really walks.  "4x2 x" is the rule that was measured and not taken: the sub-block's own slab rule
applied to the half's two rows (the region's dx interval over that slab against the half's columns).  The (splat, quadrant) and
(splat, tile) rows and the instances that reach nothing are counted as tests/sim_line0_rows.py counts them (tests/test_sim_half_groups.py holds the two scripts together on a small scene).
Usage: python tests/sim_half_groups.py [P] [slam|aniso] [batch]   (default 500000 slam 224: the K = 26 headline; ~30 s, ~3 GB)
It prints the table of EXPERIMENTS.md §10o."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "hier-slam_amd")]

W, H, K = 1200, 680, 4   # the lists and the masks do not depend on K
f = np.float32


def load(P, kind, w=W, h=H):
    """the oracle's instance list of a synthetic scene: per instance its tile, list position, tile origin, centre, conic and opacity"""
    import oracle_lib as O
    from hsr_utils.camera import replica_intrinsics, setup_camera_tensors
    from hsr_utils.synthetic import make_scene
    k = replica_intrinsics(w, h)
    cam = setup_camera_tensors(w, h, k, np.eye(4))
    sc = make_scene(P, w, h, K, k, seed=0, kind=kind)
    _, st = O.forward(cam, sc["means3D"], sc["opacities"], colors_precomp=sc["colors_precomp"], semantics_precomp=sc["semantics_precomp"],
                      scales=sc["scales"], rotations=sc["rotations"])
    try:
        m2, co = np.array(st.field("means2D")), np.array(st.field("conic_opacity"))
        keys, vals = np.array(st.field("keys")), np.array(st.field("vals"))
        ranges = np.array(st.field("ranges")).reshape(-1, 2).astype(np.int64)
        n_contrib = np.array(st.field("n_contrib")).reshape(h, w).astype(np.int64)
    finally:
        st.free()
    tiles = (keys >> np.uint64(32)).astype(np.int64)
    g = vals.astype(np.int64)
    tiles_x, tiles_y = (w + 15) // 16, (h + 15) // 16
    d = dict(W=w, H=h, tiles_x=tiles_x, tiles_y=tiles_y, tiles=tiles, ranges=ranges, n_contrib=n_contrib,
             pos=np.arange(len(g), dtype=np.int64) - ranges[tiles, 0],
             tx=((tiles % tiles_x) * 16).astype(f), ty=((tiles // tiles_x) * 16).astype(f), x=m2[g, 0].astype(f), y=m2[g, 1].astype(f))
    d["A"], d["B"], d["C"], d["o"] = [co[g, i].astype(f) for i in range(4)]
    return d


def slab_masks(d):
    """hsr_tile_common.h in numpy: sub[R, 4, 4] = subblock_mask's bit of sub-block (row r, column c) of the instance's tile,
    half[R, 8, 4] = subblock_half_mask's bit of the half-block (half-row hr = 2 r + h: pixel rows 2 hr and 2 hr + 1, column c), and
    half_x[R, 8, 4] = the same under the rule not taken (the dx interval over the half's own slab)"""
    A, B, C, o = d["A"], d["B"], d["C"], d["o"]
    t255 = f(255) * o
    ok = t255 >= 1
    with np.errstate(all="ignore"):
        tau = f(2) * np.log(np.maximum(t255, 1)).astype(f) * f(1.002) + f(0.02)
        det = A * C - B * B
        every = ok & ~((det > 0) & (A > 0) & (C > 0))   # degenerate conic: every sub-block and every half
        inv_a = f(1) / A
        hy = np.sqrt(tau * A * (f(1) / det)) * f(1.001) + f(0.02)
        dyp, atau, nb = -(B / C) * np.sqrt(tau * C * (f(1) / det)), A * tau, -B
        rx, ry = d["x"] - d["tx"], d["y"] - d["ty"]

        def span(lo_px, hi_px):
            """the slab of pixel rows lo_px .. hi_px: is it inside E's extent, and E's dx interval over it"""
            lo, hi = np.maximum(ry - f(hi_px), -hy), np.minimum(ry - f(lo_px), hy)
            top = np.maximum(lo, hi)
            dyu, dyl = np.clip(dyp, lo, top), np.clip(-dyp, lo, top)
            xmax = (nb * dyu + np.sqrt(np.maximum(atau - det * dyu * dyu, 0))) * inv_a + f(0.02)
            xmin = (nb * dyl - np.sqrt(np.maximum(atau - det * dyl * dyl, 0))) * inv_a - f(0.02)
            return (lo <= hi) & ok, xmin, xmax

        R = len(A)
        sub, half, half_x = np.zeros((R, 4, 4), bool), np.zeros((R, 8, 4), bool), np.zeros((R, 8, 4), bool)
        for r in range(4):
            on, xmin, xmax = span(4 * r, 4 * r + 3)
            for c in range(4):
                sub[:, r, c] = every | (on & ((rx - f(4 * c + 3)) <= xmax) & ((rx - f(4 * c)) >= xmin))
            for h in range(2):
                on, xmin, xmax = span(4 * r + 2 * h, 4 * r + 2 * h + 1)
                for c in range(4):
                    half[:, 2 * r + h, c] = sub[:, r, c] & (every | on)
                    half_x[:, 2 * r + h, c] = sub[:, r, c] & (every | (on & ((rx - f(4 * c + 3)) <= xmax) & ((rx - f(4 * c)) >= xmin)))
    return sub, half, half_x


def pixel_reach(d, chunk=32768):
    """acc[R, 16, 16]: does the tile's pixel (row, column) accept the instance (the forward's test: power <= 0, alpha >= 1/255)?
    Yielded a chunk of instances at a time as (slice, acc)."""
    R = len(d["A"])
    px = np.arange(16, dtype=f)
    for s in range(0, R, chunk):
        e = slice(s, min(s + chunk, R))
        dx = (d["x"][e] - d["tx"][e])[:, None, None] - px[None, None, :]
        dy = (d["y"][e] - d["ty"][e])[:, None, None] - px[None, :, None]
        A, B, C, o = [d[n][e][:, None, None] for n in "ABCo"]
        power = f(-0.5) * (A * dx * dx + C * dy * dy) - B * dx * dy
        with np.errstate(all="ignore"):
            alpha = np.minimum(f(0.99), o * np.exp(np.minimum(power, 0)))
        yield e, (power <= 0) & (alpha >= f(1.0 / 255.0))


def fold(acc, gh, gw):
    """acc[n, 16, 16] -> [n, 4 waves, groups per wave]: does a group of gh x gw pixels hold an accepting pixel?  Groups are numbered
    row-major inside the wave's 8x8 quadrant; wave = 2 * (lower half) + (right half)."""
    n = acc.shape[0]
    a = acc.reshape(n, 16 // gh, gh, 16 // gw, gw).any(axis=(2, 4))            # [n][group row][group column] of the tile
    ny, nx = 8 // gh, 8 // gw
    return a.reshape(n, 2, ny, 2, nx).transpose(0, 1, 3, 2, 4).reshape(n, 4, ny * nx)


def trips(member, tiles, n_tiles):
    """member[R, 4, G] -> (group visits, mean trips per tile and wave, mean trips of a tile's slowest wave), lists taken whole"""
    _, nw, G = member.shape
    length = np.zeros((n_tiles, nw, G), np.int64)
    for w_ in range(nw):
        for g_ in range(G):
            length[:, w_, g_] = np.bincount(tiles, weights=member[:, w_, g_], minlength=n_tiles).astype(np.int64)
    wave = length.max(axis=2)
    return int(length.sum()), float(wave.mean()), float(wave.max(axis=1).mean())


def line0_rows(d, sub, batch):
    """tests/sim_line0_rows.py's counts from the same masks: (instance, quadrant) rows the backward sends, rows per (instance, tile), and
    the instances that reach no sub-block"""
    tiles, pos = d["tiles"], d["pos"]
    R = len(tiles)
    quad = sub.reshape(R, 2, 2, 2, 2).any(axis=(2, 4)).reshape(R, 4)   # [2 * (lower half) + (right half)]
    nc = np.zeros((d["tiles_y"] * 16, d["tiles_x"] * 16), np.int64)
    nc[:d["H"], :d["W"]] = d["n_contrib"]
    ncq = nc.reshape(d["tiles_y"], 2, 8, d["tiles_x"], 2, 8).max(axis=(2, 5)).transpose(0, 2, 1, 3).reshape(-1, 4)
    hi_all = ncq.max(axis=1)
    staged = pos < hi_all[tiles]
    batch_lo = hi_all[tiles] - ((hi_all[tiles] - 1 - pos) // batch + 1) * batch
    visits = staged[:, None] & quad & (np.maximum(batch_lo, 0)[:, None] < ncq[tiles])
    return int(visits.sum()), int(visits.any(axis=1).sum()), int((~quad.any(axis=1)).sum())


def count(d, batch=224):
    """every figure the script prints, as a dict"""
    tiles, n_tiles = d["tiles"], d["tiles_x"] * d["tiles_y"]
    R = len(tiles)
    sub, half, half_x = slab_masks(d)
    shapes = {"4x4": (4, 4), "4x2": (2, 4), "2x4": (4, 2), "2x2": (2, 2)}   # name (wide x high) -> (rows, columns) of a group
    member = {n: np.zeros((R, 4, 64 // (gh * gw)), bool) for n, (gh, gw) in shapes.items()}
    for e, acc in pixel_reach(d):
        for n, (gh, gw) in shapes.items():
            member[n][e] = fold(acc, gh, gw)
    out = {"instances": R, "pixel": {n: trips(m, tiles, n_tiles) for n, m in member.items()}}
    # the kernel's own lists, in the same [wave][group] arrangement: a bit per group, expanded to the group's pixels and folded again
    sub_px = np.repeat(np.repeat(sub, 4, axis=1), 4, axis=2)
    half_px = np.repeat(np.repeat(half, 2, axis=1), 4, axis=2)
    out["slab"] = {"4x4": trips(fold(sub_px, 4, 4), tiles, n_tiles), "4x2": trips(fold(half_px, 2, 4), tiles, n_tiles),
                   "4x2 x": trips(fold(np.repeat(np.repeat(half_x, 2, axis=1), 4, axis=2), 2, 4), tiles, n_tiles)}
    out["neither_half"] = int((sub & ~half[:, 0::2] & ~half[:, 1::2]).sum())
    out["sub_entries"] = int(sub.sum())
    # a half the slab rule drops must hold no accepting pixel (the rule is conservative)
    out["half_misses"] = int((member["4x2"] & ~fold(half_px, 2, 4)).sum()) + int((half_x & ~half).sum())
    out["rows_q"], out["rows_t"], out["reach_none"] = line0_rows(d, sub, batch)
    return out


def main():
    P = int(sys.argv[1]) if len(sys.argv) > 1 else 500000
    kind = sys.argv[2] if len(sys.argv) > 2 else "slam"
    batch = int(sys.argv[3]) if len(sys.argv) > 3 else 224
    c = count(load(P, kind), batch)
    print("%s scene, P = %d, %d x %d, backward batches of %d" % (kind, P, W, H, batch))
    print("list instances (num_rendered)                                   %9d" % c["instances"])
    print("  of which reach no sub-block of their tile                     %9d (%.1f %%)" % (c["reach_none"], 100.0 * c["reach_none"] / c["instances"]))
    print("(instance, quadrant) rows the kernel sends                      %9d" % c["rows_q"])
    print("rows if sent once per (instance, tile)                          %9d" % c["rows_t"])
    print("4x4 sub-block entries (subblock_mask)                           %9d" % c["sub_entries"])
    print("  of which neither 4x2 half is reached (subblock_half_mask)     %9d" % c["neither_half"])
    print("halves with an accepting pixel that the kernel's rule drops     %9d (must be 0)" % c["half_misses"])
    for rule, title in (("pixel", "visit rule: the group holds a pixel centre with alpha >= 1/255"),
                        ("slab", "visit rule: the kernel's slab tests (subblock_mask, subblock_half_mask)")):
        print("\n" + title)
        print("| group shape | groups per wave | group visits | wave trips per tile and wave | slowest wave per tile |")
        print("|---|---|---|---|---|")
        base = c[rule]["4x4"]
        for n in ("4x4", "4x2", "4x2 x", "2x4", "2x2"):
            if n not in c[rule]:
                continue
            v, tw, ts = c[rule][n]
            rel = "" if n == "4x4" else " (%+.1f %%)" % (100.0 * (tw / base[1] - 1.0))
            rel_s = "" if n == "4x4" else " (%+.1f %%)" % (100.0 * (ts / base[2] - 1.0))
            print("| %s | %d | %.2f M | %.1f%s | %.1f%s |" % (n, {"4x4": 4, "4x2": 8, "4x2 x": 8, "2x4": 8, "2x2": 16}[n], v / 1e6, tw, rel, ts, rel_s))


if __name__ == "__main__":
    main()
