"""-m gpu: the gradient sink on the device (diff_gaussian_rasterization/_C.py set_gradient_sink, hsr_utils/parallel.py GradientExchange),
one process and one rank — no collective runs here; the exchange decisions are tested over gloo in test_parallel.py.

What the sink changes for a kernel is WHERE its outputs live: a slice of a communication bucket that starts at any float, that holds the
previous step's sums when the kernel writes it, and into which autograd adds the later keyframes of the step.  The fused input preparation
(hsr_frame_prep.hip) writes four parameter gradients there under the "params.*" names; its quaternion rows move as one 16-byte access only
where every such pointer of the launch is 16-byte aligned (include/hsr_frame_prep.h), as four floats otherwise — with the same bits."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_bwd_unpack import _OffsetSink

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
pytestmark = pytest.mark.gpu

PARAM_KEYS = ("means3D", "unnorm_rotations", "logit_opacities", "log_scales")
ROT_PARAMS, ROT_TRANSFORMED = 0, 1


class _ParamSink(_OffsetSink):
    """_OffsetSink under the names of the fused input preparation"""

    def check(self, grads):
        assert set(self.bufs) == {"params." + k for k in PARAM_KEYS}, sorted(self.bufs)
        for name, (buf, n) in self.bufs.items():
            b = buf.cpu().numpy()
            assert (b[:self.off] == self.SENTINEL).all(), "%s: floats in front of the view were written" % name
            assert (b[self.off + n:] == self.SENTINEL).all(), "%s: floats behind the view were written" % name
            g = grads[name.replace("params.", "")]
            assert np.array_equal(b[self.off:self.off + n].view(np.uint32), g.reshape(-1).view(np.uint32)), "%s: not what the view holds" % name


def _w2c():
    import frame_prep_oracle as O
    w = np.eye(4, dtype=np.float32)
    w[:3, :3] = O._rotation(np.array([0.9, 0.1, -0.3, 0.2], np.float32))[0]
    w[:3, 3] = (0.1, -0.2, 0.3)
    return w


def _offset_view(src, off, dev):
    """a contiguous copy of `src` that starts `off` floats into a 16-byte aligned buffer"""
    buf = torch.zeros(src.numel() + 8, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + src.numel()].view(src.shape)
    v.copy_(src)
    return v


def _prep_inputs(P, S, with_sil, dev):
    """inputs of one frame-prep call and fixed upstream gradients of which about 30 % of the rows are all zero (Gaussians no pixel saw)"""
    from test_frame_prep import make_grads, make_inputs
    inp = make_inputs(P, S, frames=4, seed=P + S)
    up = make_grads(P, with_sil, seed=7)
    unseen = np.random.default_rng(P).random(P) < 0.3
    if P == 1:
        unseen[:] = False
    for v in up.values():
        v[unseen] = 0.0
    return inp, up, unseen


def _prep_backward(inp, up, rot_source, w2c, dev, off=0):
    """transform_to_frame, its bundle, backward with the fixed upstream gradients.  off != 0: unnorm_rotations and the upstream gradients
    of the two quaternion outputs are views `off` floats into their buffers, so the loads are off 16 bytes as well as the stores."""
    from hsr_utils import slam_helpers as SH
    t = {k: torch.tensor(v, device=dev) for k, v in inp.items()}
    if off:
        t["unnorm_rotations"] = _offset_view(t["unnorm_rotations"], off, dev)
    t = {k: v.detach().requires_grad_(True) for k, v in t.items()}
    assert t["unnorm_rotations"].data_ptr() % 16 == (4 * off) % 16
    tg = SH.transform_to_frame(t, 2, gaussians_grad=True, camera_grad=True)
    b = tg.bundle(rot_source, None if w2c is None else torch.tensor(w2c, device=dev))
    keys = ["means3D", "unnorm_rotations", "rotations", "opacities", "scales"] + (["depth_sil"] if w2c is not None else [])
    ups = []
    for k in keys:
        g = torch.tensor(up[k], device=dev)
        ups.append(_offset_view(g, off, dev) if off and k in ("unnorm_rotations", "rotations") else g)
    torch.autograd.backward([b[k] for k in keys], ups)
    torch.cuda.synchronize()
    fwd = {k: b[k].detach().cpu().numpy() for k in keys}
    grads = {k: t[k].grad.cpu().numpy() for k in PARAM_KEYS + ("cam_unnorm_rots", "cam_trans")}
    return fwd, grads


def _same_bits(what, a, b):
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


@pytest.mark.parametrize("with_sil", [False, True])
@pytest.mark.parametrize("rot_source", [ROT_PARAMS, ROT_TRANSFORMED])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("P", [1, 255, 257, 600])
def test_frame_prep_writes_into_a_dirty_sink_at_any_float_offset(P, S, rot_source, with_sil):
    """_FramePrep alone (no rasterizer: the arithmetic is per Gaussian and repeatable), its four parameter gradients sunk into views that
    start 0, 1, 2 and 3 floats into sentinel-filled buffers: the same bits as without a sink, nothing written outside the views, exact
    zero rows for all-zero upstream rows, and the pose gradients — the reduction over all Gaussians — the same bits too."""
    from diff_gaussian_rasterization import _C
    dev = torch.device("cuda:0")
    w2c = _w2c() if with_sil else None
    inp, up, unseen = _prep_inputs(P, S, with_sil, dev)
    fwd0, plain = _prep_backward(inp, up, rot_source, w2c, dev)
    for k in PARAM_KEYS:
        assert np.isfinite(plain[k]).all() and (P == 1 or plain[k].any()), k
        assert not plain[k][unseen].any(), "%s: an all-zero upstream row gave a gradient" % k
    for off in (0, 1, 2, 3):
        sink = _ParamSink(off)
        prev = _C.set_gradient_sink(sink)
        try:
            fwd, got = _prep_backward(inp, up, rot_source, w2c, dev, off)
        finally:
            _C.set_gradient_sink(prev)
        sink.check(got)
        for k in fwd0:
            _same_bits("forward %s with unnorm_rotations %d floats off" % (k, off), fwd[k], fwd0[k])
        for k in plain:
            _same_bits("%s at float offset %d" % (k, off), got[k], plain[k])
        for k in PARAM_KEYS:
            assert not got[k][unseen].any(), "%s at float offset %d: an all-zero upstream row gave a gradient" % (k, off)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("P", [1, 257, 600])
def test_frame_prep_forward_rows_at_any_float_offset(P, S):
    """the forward through the C ABI, which is where its quaternion outputs can be given off 16 bytes: out_unnorm_rot and out_rotations
    (and the unnorm_rotations it reads) 1, 2 and 3 floats into sentinel-filled buffers — the same bits, nothing written outside"""
    from diff_gaussian_rasterization import _abi
    dev = torch.device("cuda:0")
    inp, _, _ = _prep_inputs(P, S, False, dev)
    t = {k: torch.tensor(v, device=dev) for k, v in inp.items()}
    SENT, M = -12345.5, 8

    def run(off):
        rot_in = _offset_view(t["unnorm_rotations"], off, dev)
        bufs = [torch.full((4 * P + 2 * M,), SENT, device=dev) for _ in range(2)]
        out_tr, out_rot = (b[off:off + 4 * P] for b in bufs)
        out_means, out_op, out_sc = torch.empty(P, 3, device=dev), torch.empty(P, 1, device=dev), torch.empty(P, 3, device=dev)
        assert bufs[0].data_ptr() % 16 == 0 and out_tr.data_ptr() % 16 == (4 * off) % 16
        _abi.call(_abi.lib.hsr_frame_prep_forward, "hsr_frame_prep_forward", dev, P, S, int(S != 1), ROT_TRANSFORMED, t["means3D"].data_ptr(),
                  rot_in.data_ptr(), t["logit_opacities"].data_ptr(), t["log_scales"].data_ptr(), t["cam_unnorm_rots"].data_ptr(),
                  t["cam_trans"].data_ptr(), 4, 2, None, out_means.data_ptr(), out_tr.data_ptr(), out_rot.data_ptr(), out_op.data_ptr(),
                  out_sc.data_ptr(), None)
        torch.cuda.synchronize()
        for b in bufs:
            h = b.cpu().numpy()
            assert (h[:off] == SENT).all() and (h[off + 4 * P:] == SENT).all(), "floats outside the view were written at offset %d" % off
        return [x.cpu().numpy() for x in (out_tr, out_rot, out_means, out_op, out_sc)]
    aligned = run(0)
    assert all(np.isfinite(a).all() for a in aligned)
    for off in (1, 2, 3):
        for i, (a, b) in enumerate(zip(aligned, run(off))):
            _same_bits("forward output %d at float offset %d" % (i, off), b, a)


# ---- accumulation: G = 3 keyframes of the 160 x 96, K = 26 scene summed in a bucket, twice, through GradientExchange ----
W, H, K, G = 160, 96, 26, 3
POSES = [((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((0.999, 0.01, -0.03, 0.015), (0.06, -0.02, 0.03)), ((0.998, -0.02, 0.04, -0.01), (-0.05, 0.03, 0.02))]
# a gradient of the sink under the name the rasterizer knows it by: _same_up_to_atomics_order picks its bound by that name
RASTER_NAME = {"means3D": "means3D", "unnorm_rotations": "rotations", "logit_opacities": "opacities", "log_scales": "scales",
               "rgb_colors": "colors_precomp", "semantic": "semantics_precomp"}


def _accumulate(kind):
    """kind 'raster': the six leaves go straight to the rasterizer, a camera per keyframe.  kind 'params': transform_to_frame, the semantic
    rendervar builder, the rasterizer — a pose column per keyframe, P = 2501 so that every slice of the bucket but the first starts off 16
    bytes.  Raises AssertionError; returns nothing."""
    import frame_prep_oracle as O
    import scenes
    from diff_gaussian_rasterization import GaussianRasterizer_semantic, _C
    from harness import _cam_to
    from hsr_utils import slam_helpers as SH
    from hsr_utils.camera import replica_intrinsics, setup_camera_tensors
    from hsr_utils.parallel import GradientExchange
    from test_gpu_parity import _same_up_to_atomics_order
    dev = torch.device("cuda:0")
    P = 2500 if kind == "raster" else 2501
    cam, sc, up = scenes.build(W, H, P, K, seed=3, kind="aniso", scale_mult=2.0, tilt=False, behind_frac=0.3)
    upd = {n: v.to(dev) for n, v in up.items()}
    if kind == "raster":
        names = ("means3D", "colors_precomp", "semantics_precomp", "opacities", "scales", "rotations")
        leaf = {n: sc[n].to(dev).clone().requires_grad_(True) for n in names}
        sink_names = {"raster." + n: leaf[n] for n in names}
        key = {n: n for n in names}
        cams = []
        for q, t in POSES:
            w2c = np.eye(4)
            w2c[:3, :3], w2c[:3, 3] = O._rotation(np.array(q, np.float64))[0], t
            c = setup_camera_tensors(W, H, replica_intrinsics(W, H), w2c)
            c["bg"] = cam["bg"]
            cams.append(_cam_to(c, dev))

        def render(k):
            return GaussianRasterizer_semantic(cams[k])(means2D=torch.zeros(P, 3, device=dev, requires_grad=True), **leaf)

        def regulariser():
            return leaf["scales"].sum() * 1e-3
    else:
        leaf = {"means3D": sc["means3D"], "unnorm_rotations": sc["rotations"] * 1.3,
                "logit_opacities": torch.logit(sc["opacities"].clamp(1e-4, 1 - 1e-4)), "log_scales": sc["scales"].log(),
                "rgb_colors": sc["colors_precomp"], "semantic": sc["semantics_precomp"]}
        leaf = {n: v.to(dev).clone().requires_grad_(True) for n, v in leaf.items()}
        sink_names = {("params." + n if n in PARAM_KEYS else "raster." + RASTER_NAME[n]): v for n, v in leaf.items()}
        key = RASTER_NAME
        rots = torch.tensor([q for q, _ in POSES]).T.reshape(1, 4, G) * 1.1
        trans = torch.tensor([t for _, t in POSES]).T.reshape(1, 3, G)
        params = dict(leaf, cam_unnorm_rots=rots.to(dev), cam_trans=trans.to(dev))
        camd = _cam_to(cam, dev)

        def render(k):
            rv = SH.transformed_params2rendervar_semantic(params, SH.transform_to_frame(params, k, gaussians_grad=True, camera_grad=False))
            return GaussianRasterizer_semantic(raster_settings=camd)(**rv)

        def regulariser():
            return torch.exp(leaf["log_scales"]).sum() * 1e-3

    def loss(outs, scale):
        color, radii, sem, depth, median, opac = outs
        return ((color * upd["color"]).sum() + (sem * upd["semantic"]).sum() + (depth * upd["depth"]).sum()
                + (median * upd["median"]).sum() + (opac * upd["opacity"]).sum()) * scale

    # ordinary runs: each keyframe's gradients on their own, no sink, summed in keyframe order
    ref, seen = None, torch.zeros(P, dtype=torch.bool, device=dev)
    for k in range(G):
        for t in leaf.values():
            t.grad = None
        outs = render(k)
        loss(outs, 1.0).backward()
        seen |= outs[1] > 0
        ref = {n: t.grad.clone() for n, t in leaf.items()} if ref is None else {n: ref[n] + t.grad for n, t in leaf.items()}
    unseen = ~seen
    assert 0 < int(unseen.sum()) < P, "the scene needs Gaussians that no keyframe sees, and some that one does"
    for t in leaf.values():
        t.grad = None
    ex = GradientExchange(sink_names, dev, depth=1)
    prev = _C._gradient_sink
    slices = list(zip(leaf, ex.buckets[0].views))
    if kind == "params":    # slices at 3 P, 7 P, 8 P, 11 P and 14 P floats: all but the third off 16 bytes, the quaternion gradients among them
        assert [v.data_ptr() % 16 for _, v in slices] == [0, 12, 12, 0, 12, 8], "P = 2501 was chosen to put the slices off 16 bytes"

    def step(scale, reg_in=None):
        ex.begin_step()
        for k in range(G):
            outs = render(k)
            ex.add_keyframe(outs[1])
            (loss(outs, scale) + (regulariser() if k == reg_in else 0.0)).backward()
        for n, v in slices:                        # adopted from the first backward, added to in place by the other two
            assert leaf[n].grad.data_ptr() == v.data_ptr(), "%s.grad is not the bucket's slice" % n
        torch.cuda.set_sync_debug_mode("error")    # the flag must come without a wait for the device
        try:
            flag = ex.local_foreign_flag()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        return flag
    try:
        for s, scale in enumerate((1.0, 2.0)):     # step 2 writes a bucket that holds step 1's sums; twice the loss: twice the gradients
            flag = step(scale)
            assert not bool(flag), "step %d: foreign flag set although every gradient came from the rasterizer" % s
            ex.submit()
            got = dict(zip(leaf, ex.reduced(s)))
            torch.cuda.synchronize()
            _same_up_to_atomics_order({key[n]: ref[n] * scale for n in leaf}, {key[n]: got[n] for n in leaf})
            for n in leaf:
                assert not bool(got[n][unseen].any()), "step %d, %s: a Gaussian no keyframe saw has a gradient" % (s, n)
        st = ex.stats()
        assert st["zero_copy_tensors"] == 2 * len(leaf) and st["copied_tensors"] == 0 and st["keyframes"] == 2 * G, st
        flag = step(1.0, reg_in=1)                 # a regulariser on the scales in keyframe 2: non-zero on rows no keyframe saw
        assert bool(flag), "a regulariser on the scales did not set the foreign flag"
        ex.submit()
        assert ex.stats()["zero_copy_tensors"] == 3 * len(leaf) and ex.stats()["copied_tensors"] == 0
    finally:
        ex.abort()
        _C.set_gradient_sink(prev)
    assert _C._gradient_sink is prev


@pytest.mark.parametrize("kind", ["raster", "params"])
def test_three_keyframes_accumulate_in_the_bucket(kind):
    """after the three backwards of a step every leaf's .grad is still the bucket's slice and holds the sum of three ordinary runs, up
    to the order of the tile kernel's atomics (test_gpu_parity._same_up_to_atomics_order); rows no keyframe saw are exactly zero, in a
    bucket that held other sums before; local_foreign_flag() is false without a wait for the device, true with a regulariser."""
    _accumulate(kind)


def test_three_keyframes_accumulate_in_the_bucket_through_the_ctypes_glue():
    """the same through the pure-Python glue (HSR_GLUE=ctypes is read when the package is imported: a child process)"""
    code = ("import sys; sys.path[:0] = ['hier-slam_amd', 'tests']; import test_gpu_gradient_sink as t; from diff_gaussian_rasterization import _C;"
            "assert _C._ext is None; t._accumulate('raster'); t._accumulate('params'); print('ok')")
    env = dict(os.environ, HSR_GLUE="ctypes")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
