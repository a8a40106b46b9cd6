"""CPU suite: the keyframe-parallel exchange step over gloo, world_size 2.

Each rank computes the gradients of ITS keyframe (here with the CPU oracle — tests may use it; the product
path renders on the GPU) and the bucketed all-reduce must equal the serial sum over keyframes."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _keyframe(rank, behind_frac=0.0):
    """the oracle's gradients and radii of keyframe `rank`: the same Gaussians seen from a camera of its own"""
    for p in (os.path.join(ROOT, "hier-slam_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import scenes
    from harness import run_oracle
    from hsr_utils.camera import replica_intrinsics, setup_camera_tensors
    W, H, P, K = 48, 32, 120, 4
    cam, sc, up = scenes.build(W, H, P, K, seed=1, kind="aniso", scale_mult=3.0, tilt=False, grad_seed=10 + rank, behind_frac=behind_frac)
    w2c = np.eye(4)
    w2c[0, 3] = 0.02 * rank  # a different keyframe per rank, same Gaussians
    cam2 = setup_camera_tensors(W, H, replica_intrinsics(W, H), w2c)
    out, gr, st = run_oracle(cam2, sc, up, semantic=True, threads=1)
    st.free()
    names = ("means3D", "colors_precomp", "semantics_precomp", "opacities", "scales", "rotations")
    return names, [torch.tensor(gr[n]) for n in names], torch.tensor(np.asarray(out["radii"]).astype(np.int32))


def _keyframe_grads(rank):
    names, grads, _ = _keyframe(rank)
    return names, grads


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))
    from hsr_utils.parallel import GradientBucket, allreduce_gradients, shard_keyframes
    names, grads = _keyframe_grads(rank)
    params = [torch.zeros_like(g).requires_grad_(True) for g in grads]
    for p, g in zip(params, grads):
        p.grad = g.clone()
    bucket = allreduce_gradients(params)
    assert bucket.flat.numel() == sum(g.numel() for g in grads)
    # second iteration reuses the bucket
    for p, g in zip(params, grads):
        p.grad = g.clone()
    allreduce_gradients(params, bucket=bucket)
    assert shard_keyframes(range(5), rank, world) == list(range(5))[rank::world]
    # the bench's double-buffered exchange (bench.py step()): the all-reduce of step i is waited for only when its bucket is
    # packed again; every step's reduced gradients must equal the serial sum over ranks, and nothing may be left in flight
    from hsr_utils.parallel import PipelinedAllReduce
    pipe = PipelinedAllReduce([g.shape for g in grads], "cpu", depth=2)
    seen = {}
    for i in range(5):
        if i >= 2:   # bucket i % 2 is about to be reused: what it held (step i - 2) is read first
            seen[i - 2] = [v.clone() for v in pipe.reduced(i - 2)]
        pipe.submit([g * float(i + 1) for g in grads])
    for i in (3, 4):
        seen[i] = [v.clone() for v in pipe.reduced(i)]
    pipe.drain()
    assert all(w is None for w in pipe.pending)
    for i, vs in seen.items():
        for v, g in zip(vs, grads):
            tot = g.clone() * float(i + 1)
            dist.all_reduce(tot)          # the serial (blocking) sum of the same per-rank gradients
            assert torch.equal(v, tot), "pipelined bucket of step %d differs from the serial sum" % i
    # mean + asynchronous: the division happens in wait() (it used to be dropped silently)
    b = GradientBucket([(3,)], "cpu")
    b.pack([torch.full((3,), float(rank + 1))])
    h = b.all_reduce(average=True, async_op=True)
    h.wait()
    assert torch.allclose(b.flat, torch.full((3,), sum(range(1, world + 1)) / world))
    _exchange_checks(rank, world)
    if rank == 0:
        q.put([p.grad.numpy() for p in params])
    dist.barrier()
    dist.destroy_process_group()


_TOY_NAMES = {3: ("raster.means3D", "raster.semantics_precomp", "raster.opacities"),
              6: tuple("raster." + n for n in ("means3D", "colors_precomp", "semantics_precomp", "opacities", "scales", "rotations"))}


class _ToyRender(torch.autograd.Function):
    """stands in for the rasterizer's autograd node on the CPU: its backward takes its gradient outputs from the gradient sink
    exactly as diff_gaussian_rasterization/_C.py does (a fresh allocation when no sink is installed).  apply(*leaves, *gradients):
    three leaves or all six of the rasterizer (_TOY_NAMES), and the gradient the backward is to produce for each"""

    @staticmethod
    def forward(ctx, *args):
        n = len(args) // 2
        assert n in _TOY_NAMES and len(args) == 2 * n
        ctx.save_for_backward(*args[n:])
        out = (args[0] * 0).sum()
        for a in args[1:n]:
            out = out + (a * 0).sum()
        return out

    @staticmethod
    def backward(ctx, g):
        from diff_gaussian_rasterization import _C
        outs = []
        for name, src in zip(_TOY_NAMES[len(ctx.saved_tensors)], ctx.saved_tensors):
            t = _C._from_sink(name, tuple(src.shape), src.device)
            if t is None:
                t = torch.empty_like(src)
            t.copy_(src)                      # the kernel overwrites every row (zeros for the Gaussians it did not see)
            outs.append(t)
        return tuple(outs) + (None,) * len(outs)


def _exchange_checks(rank, world):
    """GradientExchange: the leaves' gradients ARE slices of the bucket after backward (nothing packed), and the visibility-sparse
    exchange of partially overlapping views equals the dense all-reduce bit for bit (two ranks: a + b)."""
    from hsr_utils.parallel import GradientExchange, allreduce_gradients
    P = 200
    gen = torch.Generator().manual_seed(100 + rank)
    leaves = {"raster.means3D": torch.zeros(P, 3, requires_grad=True), "raster.semantics_precomp": torch.zeros(P, 5, requires_grad=True),
              "raster.opacities": torch.zeros(P, 1, requires_grad=True)}
    ex = GradientExchange(leaves, "cpu", depth=2, sparse=True, dense_above=0.9)
    ref_leaves = [torch.zeros_like(t).requires_grad_(True) for t in leaves.values()]
    views = {0: [(0, 120), (0, 200), (10, 60), (0, 0)], 1: [(80, 160), (0, 200), (50, 90), (0, 0)]}      # rows each rank sees, per step
    expect_sparse = [True, False, True, True]                                             # union 160 / 200 / 80 / 0 of 200 rows
    kept = {}
    for step in range(4):
        lo, hi = views[rank][step]
        radii = torch.zeros(P, dtype=torch.int32)
        radii[lo:hi] = 3
        grads = []
        for t in leaves.values():
            g = torch.randn(t.shape, generator=gen)
            g[radii <= 0] = 0.0
            grads.append(g)
        ex.begin_step(radii)
        _ToyRender.apply(*leaves.values(), *grads).backward()
        for i, t in enumerate(leaves.values()):      # zero copy: autograd adopted the bucket's slice as .grad
            assert t.grad.data_ptr() == ex.buckets[step % 2].views[i].data_ptr(), "gradient %d was copied, not adopted" % i
        before = ex.stats()["sparse_steps"]
        ex.submit()
        assert (ex.stats()["sparse_steps"] - before == 1) == expect_sparse[step], step
        for r, g in zip(ref_leaves, grads):
            r.grad = g.clone()
        allreduce_gradients(ref_leaves)               # the dense, blocking sum of the same per-rank gradients
        kept[step] = [r.grad.clone() for r in ref_leaves]
        if step >= 1:                                 # the bucket of step - 1 is about to be reused: read it first
            for v, e in zip(ex.reduced(step - 1), kept[step - 1]):
                assert torch.equal(v, e), "sparse exchange of step %d differs from the dense sum" % (step - 1)
    for v, e in zip(ex.reduced(3), kept[3]):          # nothing visible anywhere: no collective, zeros
        assert torch.equal(v, e) and not bool(v.any())
    ex.drain()
    st = ex.stats()
    assert st["zero_copy_tensors"] == 12 and st["copied_tensors"] == 0
    assert st["sparse_steps"] == 3 and st["bytes_exchanged"] < st["bytes_dense_equivalent"]
    assert abs(st["union_fraction"] - (160 + 80 + 0) / (3 * 200)) < 1e-9
    # a run of dense steps: after `probe_after` of them the mask is only exchanged every `probe_every`-th step (same steps on every rank)
    ex2 = GradientExchange(leaves, "cpu", depth=2, sparse=True, dense_above=0.5, probe_after=2, probe_every=3)
    full = torch.full((P,), 3, dtype=torch.int32)
    for step in range(7):
        grads = [torch.randn(t.shape, generator=gen) for t in leaves.values()]
        ex2.begin_step(full)
        _ToyRender.apply(*leaves.values(), *grads).backward()
        ex2.submit()
        for r, g in zip(ref_leaves, grads):
            r.grad = g.clone()
        allreduce_gradients(ref_leaves)
        for v, r in zip(ex2.reduced(step), ref_leaves):
            assert torch.equal(v, r.grad), step
    st2 = ex2.stats()
    assert st2["masks_exchanged"] == 4 and st2["sparse_steps"] == 0, st2      # probes before steps 0, 1, 2 and 5
    half = torch.zeros(P, dtype=torch.int32); half[:40] = 3                    # the run ends when a probe finds the union sparse again
    for step in range(7, 12):
        grads = [torch.randn(t.shape, generator=gen) for t in leaves.values()]
        for g in grads:
            g[40:] = 0.0
        ex2.begin_step(half)
        _ToyRender.apply(*leaves.values(), *grads).backward()
        ex2.submit()
        for r, g in zip(ref_leaves, grads):
            r.grad = g.clone()
        allreduce_gradients(ref_leaves)
        for v, r in zip(ex2.reduced(step), ref_leaves):
            assert torch.equal(v, r.grad), step
    ex2.drain()
    assert ex2.stats()["sparse_steps"] >= 3, ex2.stats()                       # probed at the latest three steps into the sparse phase
    # a gradient that did not come through the sink (another producer) is packed, not lost
    ex.begin_step(None)
    for t in leaves.values():
        t.grad = torch.full_like(t, float(rank + 1))
    ex.submit()
    for v in ex.reduced(4):
        assert torch.equal(v, torch.full_like(v, 3.0))
    assert ex.stats()["copied_tensors"] == 3
    _accumulate_checks(rank, world, leaves, ref_leaves, gen)


def _accumulate_checks(rank, world, leaves, ref_leaves, gen):
    """One optimizer step = G keyframes per rank accumulated locally, ONE exchange (a bucket view is handed
    out once per step and name).  The result must equal the dense sum of the 2 G single-keyframe gradients BIT FOR BIT: each rank adds
    its keyframes in order in fp32 (autograd's in-place accumulation into the adopted bucket slice), then a + b over the two ranks."""
    from hsr_utils.parallel import GradientExchange, allreduce_gradients
    P = next(iter(leaves.values())).shape[0]
    ex = GradientExchange(leaves, "cpu", sparse=True, dense_above=0.9)           # depth 1: reduced() waits, nothing overlaps a later step
    G = 3
    rows = {0: [(0, 40), (30, 70), (100, 120)], 1: [(20, 60), (110, 140), (0, 10)]}  # union over 2 x 3 keyframes: [0, 70) + [100, 140) = 110 rows
    for step in range(2):
        local = [torch.zeros_like(t) for t in leaves.values()]
        ex.begin_step()
        for k in range(G):
            lo, hi = rows[rank][k]
            radii = torch.zeros(P, dtype=torch.int32)
            radii[lo:hi] = 2
            grads = []
            for t in leaves.values():
                g = torch.randn(t.shape, generator=gen)
                g[radii <= 0] = 0.0
                grads.append(g)
            ex.add_keyframe(radii)
            _ToyRender.apply(*leaves.values(), *grads).backward()
            for acc, g in zip(local, grads):
                acc += g                                  # the same fp32 additions, in the same order
        for i, t in enumerate(leaves.values()):           # still the bucket's slice after three accumulated backwards
            assert t.grad.data_ptr() == ex.buckets[0].views[i].data_ptr()
            assert torch.equal(t.grad, local[i])
        before = ex.stats()
        ex.submit()
        after = ex.stats()
        assert after["sparse_steps"] - before["sparse_steps"] == 1 and after["copied_tensors"] == before["copied_tensors"]
        for r, acc in zip(ref_leaves, local):
            r.grad = acc.clone()
        allreduce_gradients(ref_leaves)
        for v, r in zip(ex.reduced(step), ref_leaves):
            assert torch.equal(v, r.grad), "accumulate-then-exchange differs from the dense sum of the 2 x %d keyframe gradients" % G
    st = ex.stats()
    assert st["keyframes_per_step"] == G and abs(st["union_fraction"] - 110 / P) < 1e-9, st
    # two rasterizer nodes on the same leaves in ONE graph, and a second backward through it: 1 + 10 per rank, twice (was 2 and 20)
    ex.begin_step()
    ones = [torch.ones_like(t) for t in leaves.values()]
    tens = [torch.full_like(t, 10.0) for t in leaves.values()]
    full = torch.full((P,), 5, dtype=torch.int32)
    ex.add_keyframe(full)
    loss = _ToyRender.apply(*leaves.values(), *ones) + _ToyRender.apply(*leaves.values(), *tens)
    loss.backward(retain_graph=True)
    for t in leaves.values():
        assert torch.equal(t.grad, torch.full_like(t, 11.0))
    loss.backward()
    for t in leaves.values():
        assert torch.equal(t.grad, torch.full_like(t, 22.0))
    ex.submit()
    for v in ex.reduced(2):
        assert torch.equal(v, torch.full_like(v, 22.0 * world))
    # a gradient from another producer (a regulariser: non-zero on rows no keyframe saw) in a step whose union is sparse: the flag byte of the
    # mask makes EVERY rank exchange the bucket whole — the rows outside the union are summed, not left at their local value
    ex.begin_step()
    few = torch.zeros(P, dtype=torch.int32); few[:10] = 1
    grads = [torch.zeros_like(t) for t in leaves.values()]
    for g in grads:
        g[:10] = float(rank + 1)
    ex.add_keyframe(few)
    reg = sum((t * float(rank + 1)).sum() for t in leaves.values()) if rank == 0 else 0.0    # only rank 0 has the extra producer
    (_ToyRender.apply(*leaves.values(), *grads) + reg).backward()
    before = ex.stats()["foreign_dense_steps"]
    ex.submit()
    for v in ex.reduced(3):
        e = torch.full_like(v, 1.0)          # rank 0's regulariser everywhere
        e[:10] += 1.0 + 2.0                  # + both ranks' rasterizer rows
        assert torch.equal(v, e), (v[:12], e[:12])
    assert ex.stats()["foreign_dense_steps"] - before == 1
    # a step that raises leaves no sink behind
    from diff_gaussian_rasterization import _C
    try:
        with ex.step_scope():
            raise ValueError("backward failed")
    except ValueError:
        pass
    assert _C._gradient_sink is None
    ex.drain()


def test_gradient_allreduce_gloo_world2():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = q.get(timeout=240)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    expect = None
    for r in range(world):
        _, g = _keyframe_grads(r)
        expect = [a.numpy() for a in g] if expect is None else [e + a.numpy() for e, a in zip(expect, g)]
    for a, b in zip(got, expect):
        assert np.allclose(a, b, rtol=1e-6, atol=1e-6)


def test_bucket_single_process_noop():
    sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))
    from hsr_utils.parallel import GradientBucket
    b = GradientBucket([(4, 3), (4, 1)], "cpu")
    b.pack([torch.ones(4, 3), None])
    assert b.all_reduce() is None and float(b.flat.sum()) == 12.0
    assert b.views[0].shape == (4, 3) and b.views[1].shape == (4, 1)


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def test_bench_launch_command():
    """`python bench.py --gpus N` without a launcher starts N ranks under torch.distributed.run"""
    bench = _bench()
    cmd = bench.launch_command(4, ["--gpus", "4", "--steps", "7"], 29999, python="py")
    assert cmd[:3] == ["py", "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29999"
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "7"]
    assert 1024 < bench.free_port() < 65536


def test_bench_self_launch_relays_rank0_line(monkeypatch, capsys):
    """the parent relays the child's JSON line on stdout, everything else on stderr, and returns the child's exit code —
    and never calls into torch.cuda (it must stay GPU-free so that the ranks are plain children)"""
    bench = _bench()
    import torch.cuda
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("parent touched the GPU")))
    child = "print('noise'); print('{\"metric\": \"m\", \"n_gpus\": 2}')"
    monkeypatch.setattr(bench, "launch_command", lambda n, argv, port, python=None: [sys.executable, "-c", child])
    assert bench.self_launch(2, ["--gpus", "2"]) == 0
    cap = capsys.readouterr()
    assert cap.out.strip() == '{"metric": "m", "n_gpus": 2}' and "noise" in cap.err
    monkeypatch.setattr(bench, "launch_command", lambda n, argv, port, python=None: [sys.executable, "-c", "import sys; sys.exit(3)"])
    assert bench.self_launch(2, []) == 3
    monkeypatch.setattr(bench, "launch_command", lambda n, argv, port, python=None: [sys.executable, "-c", "pass"])
    assert bench.self_launch(2, []) == 1      # no line: a failure even if the child exited 0


def test_bench_rank_cpu_sets_do_not_collide():
    """each rank gets its own L3 domain on its GPU's NUMA node, whatever CPU the launcher started it on"""
    bench = _bench()
    l3 = lambda c: set(range((c // 8) * 8, (c // 8) * 8 + 8))
    numa = {r: set(range(0, 64)) if r < 4 else set(range(64, 128)) for r in range(8)}
    picks = [bench.choose_cpus(r, 8, range(128), l3, numa, start_cpu=(r * 37) % 128) for r in range(8)]
    assert all(len(p) == 8 for p in picks)
    assert len(set(picks)) == 8
    for r, p in enumerate(picks):
        assert p <= numa[r]
    # same answer wherever the rank started
    assert picks == [bench.choose_cpus(r, 8, range(128), l3, numa, start_cpu=5) for r in range(8)]
    # unknown NUMA layout: still disjoint; more ranks than domains: wraps instead of failing
    assert len(set(bench.choose_cpus(r, 8, range(128), l3, None) for r in range(8))) == 8
    assert bench.choose_cpus(3, 4, range(16), l3, None) in (frozenset(range(0, 8)), frozenset(range(8, 16)))
    # one rank: the L3 of the CPU it runs on; tiny domains: leave the affinity alone
    assert bench.choose_cpus(0, 1, range(128), l3, None, start_cpu=13) == frozenset(range(8, 16))
    assert bench.choose_cpus(0, 1, range(128), lambda c: {c}, None, start_cpu=13) is None
    assert bench.parse_cpulist("0-3,8,10-11\n") == {0, 1, 2, 3, 8, 10, 11}


# ---- GradientExchange where the ranks do NOT do the same thing: windows shorter than the world (a rank without a keyframe), a keyframe
# without radii, gradients that did not come from the rasterizer.  Every exchange decision has to come from bytes all ranks share; a rank
# that decides from its own state enters another collective than its peers, which gloo reports by aborting (and RCCL by hanging).  So every
# case below runs its ranks as spawned CPU processes over gloo, compares each step with allreduce_gradients on the same per-rank sums,
# and the parent asserts on the exit codes. ----
def _rank_main(rank, world, port, check, kw):
    import datetime
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    for p in (os.path.join(ROOT, "hier-slam_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=100))
    globals()[check](rank, world, **kw)
    dist.barrier()
    dist.destroy_process_group()


def _run_ranks(check, world, **kw):
    """`check(rank, world, **kw)` on `world` spawned gloo ranks; a rank that fails an assertion, aborts in a mismatched collective or is
    still running at the time limit shows in the exit codes"""
    ctx = mp.get_context("spawn")
    port = _bench().free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, check, kw)) for r in range(world)]
    try:
        for p in procs:
            p.start()
        procs[0].join(timeout=240)
        for p in procs[1:]:
            p.join(timeout=120)
        codes = [p.exitcode for p in procs]
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join()
    assert codes == [0] * world, "the ranks of %s exited with %s (None: still running at the time limit)" % (check, codes)


TOY_P = 200


def _toy_leaves():
    return {"raster.means3D": torch.zeros(TOY_P, 3, requires_grad=True), "raster.semantics_precomp": torch.zeros(TOY_P, 5, requires_grad=True),
            "raster.opacities": torch.zeros(TOY_P, 1, requires_grad=True)}


def _toy_keyframe(leaves, step, kf, integer, lo=None, width=20):
    """keyframe `kf` of step `step`, the same whichever rank renders it: it sees `width` rows (a seeded place unless `lo` is given) and
    its gradients are zero everywhere else, as the rasterizer's are.  integer: small integers in fp32, whose sums are exact in any order"""
    gen = torch.Generator().manual_seed(1000 * step + kf + 1)
    if lo is None:
        lo = int(torch.randint(0, TOY_P - width, (1,), generator=gen))
    radii = torch.zeros(TOY_P, dtype=torch.int32)
    radii[lo:lo + width] = 1 + kf
    grads = []
    for t in leaves.values():
        g = torch.randint(-8, 9, t.shape, generator=gen).float() if integer else torch.randn(t.shape, generator=gen)
        g[radii <= 0] = 0.0
        grads.append(g)
    return radii, grads


def _toy_step(ex, leaves, frames, no_radii=(), reg_in=None, reg_after=None, add_after=None):
    """One step of this rank: begin_step, a _ToyRender forward and backward per frame ((radii, gradients); the frames listed in
    `no_radii` call add_keyframe(None)), submit.  Other producers, each a coefficient c standing for the gradient c of sum(c * leaf) on
    EVERY row: reg_in = (k, c) adds it to the loss of frame k, reg_after = c runs it as a backward of its own after the last frame,
    add_after = c adds it to .grad in place.  Returns the rank's own sums, formed by the same fp32 additions in the same order."""
    ts = list(leaves.values())
    local = [torch.zeros_like(t) for t in ts]
    ex.begin_step()
    for k, (radii, grads) in enumerate(frames):
        ex.add_keyframe(None if k in no_radii else radii)
        loss = _ToyRender.apply(*ts, *grads)
        c = reg_in[1] if reg_in is not None and reg_in[0] == k else None
        if c is not None:
            loss = loss + sum((t * c).sum() for t in ts)
        loss.backward()
        for acc, g in zip(local, grads):
            acc += g if c is None else g + c          # autograd sums a leaf's two gradients of one backward before it accumulates
    if reg_after is not None:
        sum((t * reg_after).sum() for t in ts).backward()
        for acc in local:
            acc += reg_after
    if add_after is not None:
        for t, acc in zip(ts, local):
            t.grad.add_(torch.full_like(t, add_after))
            acc += add_after
    if frames:
        for i, t in enumerate(ts):                    # adopted by the first backward and never replaced: nothing to pack
            assert t.grad.data_ptr() == ex.buckets[ex.cur].views[i].data_ptr(), "gradient %d is no longer the bucket's slice" % i
    ex.submit()
    return local


def _dense_reference(ref_leaves, local, average=False):
    from hsr_utils.parallel import allreduce_gradients
    for r, acc in zip(ref_leaves, local):
        r.grad = acc.clone()
    allreduce_gradients(ref_leaves, average=average)
    return [r.grad.clone() for r in ref_leaves]


def _shared_counts(ex, world):
    """the counters that follow from the exchange decisions: gathered, and the same on every rank"""
    st = ex.stats()
    mine = {k: st[k] for k in ("masks_exchanged", "sparse_steps", "foreign_dense_steps")}
    got = [None] * world
    dist.all_gather_object(got, mine)
    assert all(g == got[0] for g in got), "the ranks took different decisions: %s" % (got,)
    return mine


UNEVEN_WINDOWS = (1, 0, 2, 1, 3, 4, 7, 1, 0, 2, 1)     # keyframes in the window, step by step: 0, 1, 2, 3, 4 and 7, short ones more than once


def _deal(window, rank, step, world):
    """shard_keyframes, with the ranks' places rotated from step to step so that it is not always the last ranks that go without"""
    from hsr_utils.parallel import shard_keyframes
    return shard_keyframes(window, (rank + step) % world, world)


def _check_uneven_windows(rank, world, depth):
    from hsr_utils.parallel import GradientExchange
    integer = world > 2             # three ranks: the ring's order of additions must not matter, so the sums are made exact
    leaves = _toy_leaves()
    ex = GradientExchange(leaves, "cpu", depth=depth, sparse=True, dense_above=0.9)
    ref_leaves = [torch.zeros_like(t).requires_grad_(True) for t in leaves.values()]
    kept, without, keyframes = {}, [], 0

    def compare(s):
        dense, serial, bound = kept.pop(s)
        for v, e, t, b in zip(ex.reduced(s), dense, serial, bound):
            assert torch.equal(v, e), "step %d: the sparse exchange differs from the dense all-reduce of the same sums" % s
            if integer:
                assert torch.equal(v.double(), t), "step %d: not the serial sum over the window" % s
            else:   # n <= 7 fp32 additions in another order than the serial float64 sum: (n - 1) 2^-24 sum |terms| (8 > n - 1)
                assert bool(((v.double() - t).abs() <= 8 * 2.0 ** -24 * b).all()), "step %d: not the serial sum over the window" % s

    for s, length in enumerate(UNEVEN_WINDOWS):
        window = list(range(length))
        mine = _deal(window, rank, s, world)
        without.append(frozenset(r for r in range(world) if not _deal(window, r, s, world)))
        if depth > 1 and s >= depth:
            compare(s - depth)                      # its bucket is about to be reused: read first
        local = _toy_step(ex, leaves, [_toy_keyframe(leaves, s, kf, integer) for kf in mine])
        keyframes += len(mine)
        serial = [torch.zeros(t.shape, dtype=torch.float64) for t in leaves.values()]
        bound = [torch.zeros(t.shape, dtype=torch.float64) for t in leaves.values()]
        for kf in window:
            for acc, b, g in zip(serial, bound, _toy_keyframe(leaves, s, kf, integer)[1]):
                acc += g.double()
                b += g.double().abs()
        kept[s] = (_dense_reference(ref_leaves, local), serial, bound)
        counts = _shared_counts(ex, world)
        # at most 7 x 20 of 200 rows: every step probes, finds the union sparse and has no foreign gradient
        assert counts == dict(masks_exchanged=s + 1, sparse_steps=s + 1, foreign_dense_steps=0), (s, counts)
        if depth == 1:
            compare(s)
    for s in sorted(kept):
        compare(s)
    ex.drain()
    assert all(w is None for w in ex.pending)
    st = ex.stats()
    assert st["keyframes"] == keyframes and st["steps"] == len(UNEVEN_WINDOWS), st
    assert st["copied_tensors"] == 3 * sum(1 for s, length in enumerate(UNEVEN_WINDOWS) if not _deal(list(range(length)), rank, s, world)), st
    assert st["bytes_exchanged"] < st["bytes_dense_equivalent"]
    # what this case is for: steps in which some ranks, but not all, go without a keyframe — and not always the same ranks
    some = {w for w in without if 0 < len(w) < world}
    assert len(some) >= 2 and frozenset(range(world)) in without and frozenset() in without, without


@pytest.mark.parametrize("world,depth", [(2, 1), (3, 1), (2, 2), (3, 2)])
def test_exchange_with_windows_shorter_than_the_world(world, depth):
    """Windows of 0, 1, 2, 3, 4 and 7 keyframes dealt by shard_keyframes to 2 and 3 ranks over consecutive steps: the ranks that render
    nothing change from step to step and still enter the same collectives as the others.  depth = 2: the same with two buckets, each
    step's bucket read before it is reused and nothing left pending after drain().  At the parent commit a rank without a keyframe skipped
    the mask all-reduce its peer entered, and the ranks ended with exit codes [-6, 1]."""
    _run_ranks("_check_uneven_windows", world, depth=depth)


def _check_missing_radii(rank, world):
    from hsr_utils.parallel import GradientExchange
    leaves = _toy_leaves()
    ex = GradientExchange(leaves, "cpu", sparse=True, dense_above=0.9)
    ref_leaves = [torch.zeros_like(t).requires_grad_(True) for t in leaves.values()]
    dense_bytes = ex.buckets[0].flat.numel() * 4
    # step -> (keyframes of rank 0, keyframes of rank 1, (rank, frame) that gives no radii); in step 3 the other rank has no keyframe at all
    plan = [(1, 1, None), (1, 2, (1, 1)), (2, 1, None), (1, 0, (0, 0)), (1, 1, None)]
    for s, (n0, n1, missing) in enumerate(plan):
        n = (n0, n1)[rank]
        frames = [_toy_keyframe(leaves, s, 2 * k + rank, False) for k in range(n)]
        before = ex.stats()
        local = _toy_step(ex, leaves, frames, no_radii=(missing[1],) if missing is not None and missing[0] == rank else ())
        after, counts = ex.stats(), _shared_counts(ex, world)
        for v, e in zip(ex.reduced(s), _dense_reference(ref_leaves, local)):
            assert torch.equal(v, e), s
        assert counts["masks_exchanged"] == s + 1 and counts["foreign_dense_steps"] == 0, (s, counts)
        if missing is None:        # sparse before and sparse again right after
            assert after["sparse_steps"] - before["sparse_steps"] == 1 and after["bytes_exchanged"] - before["bytes_exchanged"] < dense_bytes, s
        else:                      # EVERY rank exchanges the bucket whole, not only the one without radii
            assert after["sparse_steps"] == before["sparse_steps"] and after["bytes_exchanged"] - before["bytes_exchanged"] == dense_bytes, s


def test_exchange_when_one_keyframe_gives_no_radii():
    """add_keyframe(None) on one rank for one of its keyframes: that step is exchanged whole by every rank — the flag travels with the
    mask — and the next one is sparse again"""
    _run_ranks("_check_missing_radii", 2)


FOREIGN_KINDS = {"regulariser_in_the_loss_of_keyframe_2_of_3": dict(reg_in=1), "separate_backward_after_the_last_keyframe": dict(reg_after=True),
                 "added_to_grad_in_place_after_adoption": dict(add_after=True)}


def _check_foreign(rank, world, kind):
    from hsr_utils.parallel import GradientExchange
    leaves = _toy_leaves()
    ex = GradientExchange(leaves, "cpu", sparse=True, dense_above=0.9)
    ref_leaves = [torch.zeros_like(t).requires_grad_(True) for t in leaves.values()]
    s = 0
    for producers in ((0,), (0, 1)):                      # the other producer on one rank only, then on both
        c = float(rank + 1) if rank in producers else None
        extra = {}
        if c is not None:
            extra = {k: ((v, c) if k == "reg_in" else c) for k, v in FOREIGN_KINDS[kind].items()}
        # three keyframes per rank, all inside rows 0..19: rows 20.. are seen by nobody, and only the other producer writes them
        frames = [_toy_keyframe(leaves, s, 3 * rank + k, True, lo=3 * k + rank, width=10) for k in range(3)]
        before = ex.stats()
        local = _toy_step(ex, leaves, frames, **extra)
        after, counts = ex.stats(), _shared_counts(ex, world)
        outside = float(sum(r + 1 for r in producers))
        for v, e in zip(ex.reduced(s), _dense_reference(ref_leaves, local)):
            assert torch.equal(v[20:], torch.full_like(v[20:], outside)), \
                "row 50 holds %s, the regularisers of ranks %s sum to %s" % (v[50].tolist(), producers, outside)
            assert torch.equal(v, e)
        assert after["foreign_dense_steps"] - before["foreign_dense_steps"] == 1 and after["sparse_steps"] == before["sparse_steps"], (before, after)
        assert after["zero_copy_tensors"] - before["zero_copy_tensors"] == 3 and after["copied_tensors"] == before["copied_tensors"], (before, after)
        s += 1
        # and a step without it is sparse again
        local = _toy_step(ex, leaves, [_toy_keyframe(leaves, s, 3 * rank + k, True, lo=3 * k + rank, width=10) for k in range(3)])
        counts = _shared_counts(ex, world)
        for v, e in zip(ex.reduced(s), _dense_reference(ref_leaves, local)):
            assert torch.equal(v, e) and not bool(v[20:].any())
        assert counts["sparse_steps"] == (s + 1) // 2 and counts["foreign_dense_steps"] == (s + 1) // 2, (s, counts)
        s += 1


@pytest.mark.parametrize("kind", list(FOREIGN_KINDS))
def test_exchange_with_a_gradient_that_is_not_the_rasterizers(kind):
    """A producer whose gradient is not zero outside the visible union, contributing AFTER the first backward's view was adopted — so
    `.grad` is still the bucket's slice and no pointer tells: the step must go dense on every rank (foreign_dense_steps + 1), the rows no
    keyframe saw must hold the summed regulariser, and nothing may be copied.  At the parent commit the keyframe-2 regulariser of one
    rank left row 50 of the reduced gradient at 1.0 on that rank and 0.0 on the other, with foreign_dense_steps == 0."""
    _run_ranks("_check_foreign", 2, kind=kind)


def _check_probe_schedule(rank, world):
    from hsr_utils.parallel import GradientExchange
    leaves = _toy_leaves()
    ex = GradientExchange(leaves, "cpu", depth=1, sparse=True, dense_above=0.5, probe_after=2, probe_every=3)
    ref_leaves = [torch.zeros_like(t).requires_grad_(True) for t in leaves.values()]
    without = {1: 1, 3: 1, 4: 0, 6: 1, 7: 0, 10: 0}       # step -> the rank that has no keyframe in it
    # steps 0..9: every keyframe sees all rows.  _dense_run 0, 1: probed; from 2 on every third step: 2, 5, 8.  From step 10 on a keyframe sees
    # 40 rows, but step 10 is no probe: still dense; the probe of step 11 finds the union sparse, and the run is over.
    probes = [1, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5, 6, 7]
    sparse = [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2]
    for s in range(13):
        frames = [] if without.get(s) == rank else [_toy_keyframe(leaves, s, rank, False, lo=0, width=TOY_P if s < 10 else 40)]
        local = _toy_step(ex, leaves, frames)
        counts = _shared_counts(ex, world)
        assert counts == dict(masks_exchanged=probes[s], sparse_steps=sparse[s], foreign_dense_steps=0), (s, counts)
        for v, e in zip(ex.reduced(s), _dense_reference(ref_leaves, local)):
            assert torch.equal(v, e), s


def test_probe_schedule_is_the_same_on_a_rank_without_a_keyframe():
    """probe_after = 2, probe_every = 3 through a dense stretch in which one rank or the other has no keyframe in some steps: _dense_run
    moves by the all-reduced bytes alone, so every rank probes in the same steps — masks_exchanged, gathered step by step"""
    _run_ranks("_check_probe_schedule", 2)


def _check_sparse_average(rank, world):
    from hsr_utils.parallel import GradientExchange
    leaves = _toy_leaves()
    ex = GradientExchange(leaves, "cpu", sparse=True, dense_above=0.9, average=True)
    ref_leaves = [torch.zeros_like(t).requires_grad_(True) for t in leaves.values()]
    for s, length in enumerate((3, 1, 0, 2, 1)):
        mine = _deal(list(range(length)), rank, s, world)
        local = _toy_step(ex, leaves, [_toy_keyframe(leaves, s, kf, False) for kf in mine])
        for v, e in zip(ex.reduced(s), _dense_reference(ref_leaves, local, average=True)):
            assert torch.equal(v, e), s
        assert _shared_counts(ex, world)["sparse_steps"] == s + 1


def test_sparse_exchange_with_average_equals_the_dense_mean():
    _run_ranks("_check_sparse_average", 2)


def _check_real_gradients(rank, world):
    from hsr_utils.parallel import GradientExchange
    names, grads, radii = _keyframe(rank, behind_frac=0.3)      # part of the map behind both cameras
    P = int(radii.numel())
    for n, g in zip(names, grads):
        assert not bool(g[radii <= 0].any()), "%s: a Gaussian the keyframe did not see has a gradient" % n
    seen = [None] * world
    dist.all_gather_object(seen, (radii > 0).tolist())
    union = int(torch.tensor(seen).any(dim=0).sum())
    assert 0 < union < 0.9 * P and int((radii > 0).sum()) > 0, (union, P)
    leaves = {"raster." + n: torch.zeros_like(g).requires_grad_(True) for n, g in zip(names, grads)}
    ex = GradientExchange(leaves, "cpu", sparse=True, dense_above=0.9)
    ex.begin_step()
    ex.add_keyframe(radii)
    _ToyRender.apply(*leaves.values(), *grads).backward()
    ex.submit()
    ref_leaves = [torch.zeros_like(g).requires_grad_(True) for g in grads]
    for n, v, e in zip(names, ex.reduced(0), _dense_reference(ref_leaves, grads)):
        assert torch.equal(v, e), n
    st = ex.stats()
    assert st["sparse_steps"] == 1 and st["union_rows"] == union and st["foreign_dense_steps"] == 0 and st["zero_copy_tensors"] == 6, st


def test_sparse_exchange_of_the_oracles_gradients_with_its_own_radii():
    """the two oracle keyframes (different cameras, 30 % of the map behind them) with the oracle's radii as the visibility: every row with
    radii <= 0 is exactly zero in all six gradients, the union is smaller than P, and the sparse exchange equals the dense sum bit for bit"""
    _run_ranks("_check_real_gradients", 2)


def test_local_foreign_flag_reads_the_bucket_not_the_pointers():
    """one rank, no process group: the flag is a device scalar, true where a row outside the rank's own mask holds anything but zero —
    NaN counts, -0.0 does not — and without a keyframe every row is outside"""
    sys.path.insert(0, os.path.join(ROOT, "hier-slam_amd"))
    from hsr_utils.parallel import GradientExchange
    leaves = _toy_leaves()
    ex = GradientExchange(leaves, "cpu", sparse=True)
    with pytest.raises(RuntimeError):
        ex.local_foreign_flag()                                   # no step is open
    radii, grads = _toy_keyframe(leaves, 0, 0, False, lo=10, width=20)
    try:
        ex.begin_step()
        ex.add_keyframe(radii)
        _ToyRender.apply(*leaves.values(), *grads).backward()
        flag = ex.local_foreign_flag()
        assert isinstance(flag, torch.Tensor) and flag.dim() == 0 and flag.dtype == torch.bool and not bool(flag)
        sem = leaves["raster.semantics_precomp"].grad
        assert sem.data_ptr() == ex.buckets[0].views[1].data_ptr()
        sem[150, 3] = -0.0
        assert not bool(ex.local_foreign_flag())
        sem[15, 3] = float("nan")                                  # inside the mask: the rasterizer's own business
        assert not bool(ex.local_foreign_flag())
        sem[150, 3] = float("nan")
        assert bool(ex.local_foreign_flag())
        sem[150, 3] = 0.0
        leaves["raster.opacities"].grad[TOY_P - 1, 0] = 1e-30      # the last row of the last tensor
        assert bool(ex.local_foreign_flag())
        ex.submit()
        ex.begin_step()                                            # no keyframe: nothing is visible
        assert ex.stats()["keyframes"] == 1
        for t in leaves.values():
            t.grad = torch.zeros_like(t)
        ex.submit()
        assert ex.stats()["keyframes"] == 1 and ex.stats()["steps"] == 2    # a step without a keyframe counts none
        ex.begin_step()
        ex.buckets[0].flat.zero_()
        assert not bool(ex.local_foreign_flag())
        ex.buckets[0].flat[7] = 2.0
        assert bool(ex.local_foreign_flag())
    finally:
        ex.abort()
