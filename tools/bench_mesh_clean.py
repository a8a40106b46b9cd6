#!/usr/bin/env python3
"""Measures the removal of small components on the device (include/surface/hsr_mesh_clean.h; EXPERIMENTS.md §23): the synthetic room of
tools/bench_mesh.py (256^3 points, 964 k faces) with a cloud of small spherical shells written into its volume, extracted, then
mesh_components and clean_mesh against the eager torch chain a user would write without them:

    labels   label propagation over the edges (a, b) and (b, c) by scatter_reduce_(amin) with one pointer jump a round, until a round
             changes nothing (one host read a round); face counts by bincount
    compact  a boolean mask over the faces, the used vertices marked, a cumsum for the new indices (as mesh_eval.cull_mesh)

Times are device events around warmed-up work (the eager chain's include its host reads); ONE JSON line.

    python tools/bench_mesh_clean.py [--reps N] [--shells N] [--min-faces N]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_mesh as BM  # noqa: E402


def add_shells(vol, n, radius, seed):
    """n small spheres into the free space of the room: tsdf = min(tsdf, clamped distance) in a window of sample points around each"""
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    X, Y, Z = vol.dims
    h, reach = vol.voxel_size, int(np.ceil((radius + vol.trunc) / vol.voxel_size)) + 1
    half = np.array(BM.ROOM) - radius - 2 * vol.trunc      # clear of the walls: a shell of its own
    for centre in rng.uniform(-half, half, (n, 3)):
        c = [int(round((centre[a] - vol.origin[a]) / h)) for a in range(3)]
        lo = [max(0, c[a] - reach) for a in range(3)]
        hi = [min((X, Y, Z)[a], c[a] + reach + 1) for a in range(3)]
        axes = [vol.origin[a] + h * torch.arange(lo[a], hi[a], device=vol.device, dtype=torch.float32) - float(centre[a]) for a in range(3)]
        dist = torch.sqrt(axes[2][:, None, None] ** 2 + axes[1][None, :, None] ** 2 + axes[0][None, None, :] ** 2) - radius
        window = vol.tsdf[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
        window.copy_(torch.minimum(window, torch.clamp(dist / vol.trunc, -1.0, 1.0)))


def eager_components(faces, V):
    """(label int64 [V], face_count int64 [V]) by label propagation; also the number of rounds"""
    import torch
    f = faces.long()
    e0, e1 = torch.cat([f[:, 0], f[:, 1]]), torch.cat([f[:, 1], f[:, 2]])
    label = torch.arange(V, device=faces.device)
    rounds = 0
    while True:
        rounds += 1
        m = torch.minimum(label[e0], label[e1])
        new = label.clone()
        new.scatter_reduce_(0, e0, m, "amin")
        new.scatter_reduce_(0, e1, m, "amin")
        new = new[new]      # a label is a vertex of the same component: one pointer jump
        if torch.equal(new, label):      # the host read of the round
            break
        label = new
    return label, torch.bincount(label[f[:, 0]], minlength=V), rounds


def eager_compact(vertices, faces, rgb, labels, label, keep):
    import torch
    f = faces.long()
    kept = f[keep[label[f[:, 0]]].bool()]
    used = torch.zeros(vertices.shape[0], dtype=torch.bool, device=faces.device)
    used[kept.reshape(-1)] = True
    new_index = torch.cumsum(used.to(torch.int64), 0) - 1
    return vertices[used], new_index[kept].to(torch.int32), rgb[used], labels[used]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shells", type=int, default=400)
    ap.add_argument("--min-faces", type=int, default=5000)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_clean.py needs a GPU")
    from hsr_utils import mesh, mesh_clean
    dev = torch.device("cuda", torch.cuda.current_device())
    k = np.array([[BM.FX, 0, BM.W / 2 - 0.5], [0, BM.FX, BM.H / 2 - 0.5], [0, 0, 1]], np.float32)
    poses = [BM.rotation(ax, ay) for ax in (-0.5, 0.0, 0.5) for ay in np.linspace(0, 2 * np.pi, 4, endpoint=False)]
    dims, h = (256, 256, 256), 0.02
    room = mesh.TsdfVolume(tuple(-h * (d - 1) / 2 for d in dims), dims, h, labels=True)
    for p in poses:
        depth, colour, lab = BM.room_view(p, dev)
        room.integrate(depth, p, k, color=colour, labels=lab)
    faces_room = int(room.extract()[1].shape[0])
    add_shells(room, a.shells, 0.05, 0)
    vertices, faces, rgb, labels = room.extract()
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    t_extract = BM.timed(room.extract, 3)

    label, count = mesh_clean.mesh_components(faces, V)
    clean = lambda: mesh_clean.clean_mesh(vertices, faces, rgb, labels, min_faces=a.min_faces)
    got = clean()
    # alternately, the smaller of two: whichever is timed first would otherwise carry the clock's ramp
    t_components, t_clean = float("inf"), float("inf")
    for _ in range(2):
        t_components = min(t_components, BM.timed(lambda: mesh_clean.mesh_components(faces, V), a.reps))
        t_clean = min(t_clean, BM.timed(clean, a.reps))

    elabel, ecount, rounds = eager_components(faces, V)
    keep = mesh_clean.component_keep(ecount, min_faces=a.min_faces)
    want = eager_compact(vertices, faces, rgb, labels, elabel, keep)
    same = bool(torch.equal(elabel.int(), label) and torch.equal(ecount.int(), count) and all(torch.equal(x, y) for x, y in zip(got, want)))
    eager_reps = max(2, a.reps // 5)
    t_eager_components = BM.timed(lambda: eager_components(faces, V), eager_reps)

    def eager_clean():
        lab_, cnt_, _ = eager_components(faces, V)
        return eager_compact(vertices, faces, rgb, labels, lab_, mesh_clean.component_keep(cnt_, min_faces=a.min_faces))

    t_eager_clean = BM.timed(eager_clean, eager_reps)
    sizes = count[count > 0]
    print(json.dumps(dict(what="mesh_clean", faces=F, vertices=V, faces_of_the_room=faces_room, components=int(sizes.numel()),
                          largest=int(sizes.max()), kept_faces=int(got[1].shape[0]), kept_vertices=int(got[0].shape[0]), equal_to_eager=same,
                          eager_rounds=rounds,
                          ms=dict(extract=round(t_extract, 3), mesh_components=round(t_components, 4), clean_mesh=round(t_clean, 4),
                                  eager_components=round(t_eager_components, 3), eager_clean=round(t_eager_clean, 3)),
                          ratio=dict(components=round(t_eager_components / t_components, 1), clean=round(t_eager_clean / t_clean, 1)))), flush=True)


if __name__ == "__main__":
    main()
