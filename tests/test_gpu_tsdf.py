"""GPU suite for the mesh of a finished run (include/ext/hsr_tsdf.h): hsr_tsdf_integrate bit for bit against the numpy float32
restatement (tests/tsdf_ref.py) for every state tensor; hsr_tsdf_count / hsr_tsdf_faces / hsr_tsdf_vertices against the restatement's
surface — vertices, colours and labels bit for bit, the faces as a set of oriented triangles; the analytic sphere's conditions on the
device's own mesh; every refusal with poisoned outputs.  A poisoned tail follows every output.

Derivable, not measured: the file is built without contraction and every operation of both chains is one correctly rounded IEEE
operation in a stated order, so the expectation is equality of bits (a NaN matching a NaN)."""
import numpy as np
import pytest
import torch

import tsdf_ref as R
import test_tsdf_cpu as TC

pytestmark = pytest.mark.gpu

POISON = -777.25
POISON_INT = -77777
TAIL = 8
STATE = ("tsdf", "weight", "color", "cweight", "best", "label")
GRIDS = [(1, 1, 1), (2, 2, 2), (5, 4, 3), (17, 13, 11), (67, 9, 6), (20, 13, 11)]      # the last: four points a lane over several blocks
IMAGES = [(8, 6), (40, 30)]      # W, H
MODES = [(True, True), (True, False), (False, True), (False, False)]      # colour, labels


def _device():
    return torch.device("cuda", torch.cuda.current_device())


# ---- the calls: state and outputs with poisoned tails, at 16-byte-aligned or at odd addresses ----------------------------------------------
def _guarded(array, odd, poison):
    """a device copy of `array` with TAIL poisoned elements behind it (and, odd, one in front: the payload then starts 4 bytes off a
    16-byte boundary); returns (the whole buffer, the view of the payload)"""
    a = np.ascontiguousarray(array).reshape(-1)
    lead = 1 if odd else 0
    buf = torch.full((lead + a.size + TAIL,), poison, dtype=torch.from_numpy(a[:0].copy()).dtype, device=_device())
    assert buf.data_ptr() % 16 == 0
    buf[lead:lead + a.size] = torch.from_numpy(a.copy()).to(buf.device)
    return buf, buf[lead:lead + a.size]


def _untouched(buf, payload_size, odd, poison):
    lead = 1 if odd else 0
    return bool((buf[:lead] == poison).all() and (buf[lead + payload_size:] == poison).all())


def _integrate(vol, view, odd=False):
    """hsr_tsdf_integrate through the C ABI on a device copy of vol's state; returns the new state as numpy arrays"""
    from diff_gaussian_rasterization import _abi
    dev = _device()
    state = vol.state()
    bufs = {n: _guarded(a, odd, POISON_INT if n == "label" else POISON) for n, a in state.items()}
    depth = torch.from_numpy(view["depth"]).to(dev)
    H, W = view["depth"].shape
    image = None if view.get("image") is None else torch.from_numpy(view["image"]).to(dev)
    labels = None if view.get("labels") is None else torch.from_numpy(view["labels"]).to(dev)
    opacity = None if view.get("opacity") is None else torch.from_numpy(view["opacity"]).to(dev)
    k = view["k"]
    w2c = np.ascontiguousarray(view["w2c"], np.float32)
    ptr = lambda n: bufs[n][1].data_ptr() if n in bufs else None
    tp = lambda t: None if t is None else t.data_ptr()
    _abi.call(_abi.lib.hsr_tsdf_integrate, "hsr_tsdf_integrate", dev, vol.X, vol.Y, vol.Z, *[float(o) for o in vol.origin], float(vol.h),
              float(vol.trunc), float(vol.max_weight), H, W, float(k[0][0]), float(k[1][1]), float(k[0][2]), float(k[1][2]),
              w2c.ctypes.data_as(_abi.fp), depth.data_ptr(), tp(image), tp(labels), tp(opacity), float(view.get("sil_thres", 0.0)),
              float(view.get("depth_max", 0.0)), *[ptr(n) for n in STATE])
    torch.cuda.synchronize()
    for n, (buf, _payload) in bufs.items():
        assert _untouched(buf, state[n].size, odd, POISON_INT if n == "label" else POISON), "written outside %s" % n
    return {n: payload.cpu().numpy().reshape(state[n].shape) for n, (_buf, payload) in bufs.items()}


def _surface(vol, odd=False):
    """hsr_tsdf_count, the running sum, hsr_tsdf_faces, torch.unique and hsr_tsdf_vertices through the C ABI, every output guarded;
    returns (counts, keys [T,3], vertex keys, faces int32 [T,3], positions, rgb | None, labels | None) as numpy arrays"""
    from diff_gaussian_rasterization import _abi
    dev = _device()
    N = vol.N
    tsdf, weight = torch.from_numpy(vol.tsdf).to(dev), torch.from_numpy(vol.weight).to(dev)
    cbuf, counts = _guarded(np.full(N, POISON_INT, np.int32), odd, POISON_INT)
    _abi.call(_abi.lib.hsr_tsdf_count, "hsr_tsdf_count", dev, vol.X, vol.Y, vol.Z, tsdf.data_ptr(), weight.data_ptr(), counts.data_ptr())
    assert _untouched(cbuf, N, odd, POISON_INT) and (counts >= 0).all()
    offsets = torch.cumsum(counts, 0, dtype=torch.int64)
    T = int(offsets[-1])
    kbuf, keys = _guarded(np.full(3 * T, POISON_INT, np.int64), odd, POISON_INT)
    _abi.call(_abi.lib.hsr_tsdf_faces, "hsr_tsdf_faces", dev, vol.X, vol.Y, vol.Z, tsdf.data_ptr(), weight.data_ptr(), offsets.data_ptr(), T,
              keys.data_ptr() if T else None)
    assert _untouched(kbuf, 3 * T, odd, POISON_INT) and (keys > 0).all()      # every row written: no key is 0 (direction >= 1)
    vkeys, inverse = torch.unique(keys, return_inverse=True)
    V = int(vkeys.numel())
    color = None if vol.color is None else torch.from_numpy(vol.color).to(dev)
    cweight = None if vol.color is None else torch.from_numpy(vol.cweight).to(dev)
    label = None if vol.label is None else torch.from_numpy(vol.label).to(dev)
    pbuf, pos = _guarded(np.full(3 * V, POISON, np.float32), odd, POISON)
    rbuf, rgb = _guarded(np.full(3 * V, 0xA5, np.uint8), odd, 0xA5)
    lbuf, lab = _guarded(np.full(V, POISON_INT, np.int32), odd, POISON_INT)
    tp = lambda t: None if t is None else t.data_ptr()
    _abi.call(_abi.lib.hsr_tsdf_vertices, "hsr_tsdf_vertices", dev, vol.X, vol.Y, vol.Z, *[float(o) for o in vol.origin], float(vol.h), V,
              vkeys.data_ptr() if V else None, tsdf.data_ptr(), tp(color), tp(cweight), tp(label), pos.data_ptr() if V else None,
              rgb.data_ptr() if V and color is not None else None, lab.data_ptr() if V and label is not None else None)
    torch.cuda.synchronize()
    assert _untouched(pbuf, 3 * V, odd, POISON) and _untouched(rbuf, 3 * V, odd, 0xA5) and _untouched(lbuf, V, odd, POISON_INT)
    if color is None:
        assert (rgb == 0xA5).all()
    if label is None:
        assert (lab == POISON_INT).all()
    return (counts.cpu().numpy(), keys.cpu().numpy().reshape(T, 3), vkeys.cpu().numpy(), inverse.reshape(T, 3).to(torch.int32).cpu().numpy(),
            pos.cpu().numpy().reshape(V, 3), None if color is None else rgb.cpu().numpy().reshape(V, 3), None if label is None else lab.cpu().numpy())


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------
def _rotation(axis, degrees):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    t = np.deg2rad(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def _w2c(rot, trans):
    m = np.eye(4, dtype=np.float32)
    m[:3, :3], m[:3, 3] = rot, trans
    return m


def _volume(dims, max_weight, colour, labels):
    """a volume 0.7 in front of the first camera, centred on its axis (off by a few millimetres: no sample point on a pixel border)"""
    X, Y, Z = dims
    h = 0.1
    return R.Volume((-h * (X - 1) / 2 + 0.013, -h * (Y - 1) / 2 - 0.007, 0.7), dims, h, 0.25, max_weight, color=colour, labels=labels)


def _views(dims, W, H, colour, labels, seed):
    """three views: the first camera; a tilted one with a depth limit and an opacity mask with values at the threshold; one that
    stands inside the volume, so that part of it is behind the camera"""
    g = np.random.default_rng(seed)
    Z = dims[2]
    k = np.array([[0.75 * W, 0, W / 2 - 0.37], [0, 0.75 * W, H / 2 + 0.21], [0, 0, 1]], np.float32)
    poses = [np.eye(4, dtype=np.float32), _w2c(_rotation([0.3, 1.0, 0.2], 7.0), (0.05, -0.03, 0.08)),
             _w2c(_rotation([1.0, -0.2, 0.1], -5.0), (0.02, 0.01, -(0.7 + 0.1 * (Z - 1) / 2)))]
    views = []
    for n, w2c in enumerate(poses):
        depth = (g.random((H, W)) * (0.5 + 0.1 * Z) + (0.5 if n < 2 else 0.02)).astype(np.float32)
        flat = depth.reshape(-1)
        for q, v in enumerate((0.0, np.nan, np.inf, -1.25, -0.0, -np.inf)):      # planted: none of them is a depth
            flat[(5 * q + 3 * n + 1) % flat.size] = v
        view = dict(depth=depth, w2c=w2c, k=k)
        if colour:
            view["image"] = g.random((3, H, W)).astype(np.float32)
        if labels:
            view["labels"] = g.integers(0, 100000, (H, W)).astype(np.int64)      # beyond 16 bits
            view["labels"].reshape(-1)[::7] = 2 ** 16 + n
        if n == 1:
            view["depth_max"] = 1.1
            thr = np.float32(0.5)
            opacity = g.random((H, W)).astype(np.float32)
            opacity.reshape(-1)[::3] = thr                             # at the threshold: does not count
            opacity.reshape(-1)[1::3] = np.nextafter(thr, np.float32(1))      # one ulp above: counts
            opacity.reshape(-1)[2::9] = np.nextafter(thr, np.float32(0))
            view["opacity"], view["sil_thres"] = opacity, 0.5
        views.append(view)
    return views


def _same_state(got, want, what):
    assert set(got) == set(want), what
    for n in want:
        if want[n].dtype == np.int32:
            assert got[n].dtype == np.int32 and np.array_equal(got[n], want[n]), (n, what)
        else:
            assert R.same_floats(got[n], want[n]), (n, what, np.argwhere(got[n].view(np.uint32) != want[n].view(np.uint32))[:5])


def _ref_integrate(vol, view):
    return R.integrate(vol, view["depth"], view["w2c"], view["k"], image=view.get("image"), labels=view.get("labels"),
                       opacity=view.get("opacity"), sil_thres=view.get("sil_thres", 0.0), depth_max=view.get("depth_max", 0.0))


_fused = {}      # (dims, image): the restatement's volume after the three views with colour and labels — computed once, never changed


@pytest.mark.parametrize("W,H", IMAGES)
@pytest.mark.parametrize("dims", GRIDS)
def test_integrate_equals_the_restatement_bit_for_bit(dims, W, H):
    seed = 1000 * dims[0] + 10 * dims[1] + W
    for colour, labels in MODES:
        vol = _volume(dims, 2.0, colour, labels)      # max_weight = 2: the third view meets the cap
        for n, view in enumerate(_views(dims, W, H, colour, labels, seed)):
            before = vol.copy()
            _ref_integrate(vol, view)
            for odd in (False, True):      # four points a lane where X*Y*Z % 4 == 0 and the state is 16-byte aligned, else one
                got = _integrate(before, view, odd)
                _same_state(got, vol.state(), (dims, W, H, colour, labels, n, odd))
        if vol.N > 2000:      # the wide grids reach beyond the image: the cap was met, part of the volume was never seen
            assert vol.weight.max() == 2 and (vol.weight == 0).any() and (vol.weight == 1).any()
            if colour:
                assert 0 < (vol.cweight > 0).sum() < (vol.weight > 0).sum()      # the band is narrower than the view
            if labels:
                assert vol.label.max() >= 2 ** 16 and (vol.label == -1).any()
        if colour and labels:
            _fused[(dims, W, H)] = vol


def test_integrate_with_state_but_no_image_leaves_colour_and_labels():
    dims = (17, 13, 11)
    view = _views(dims, 40, 30, False, False, 5)[0]
    vol = _volume(dims, 64.0, True, True)
    got = _integrate(vol, view)
    _ref_integrate(vol, view)
    _same_state(got, vol.state(), "no image")
    assert not got["color"].any() and not got["cweight"].any() and (got["label"] == -1).all() and np.isinf(got["best"]).all()
    assert (got["weight"] == 1).any()


def test_integrate_at_exact_edges():
    """sample points whose pixel centre falls exactly on the image border, and sdf == -trunc exactly: every number below is a dyadic
    fraction, so the chain is exact and the expectation can be written down"""
    vol = R.Volume((-0.5, -0.5, 1.0), (3, 3, 2), 0.5, 0.25, 64.0, color=True, labels=True)
    W, H = 8, 6
    k = np.array([[8.0, 0, 3.5], [0, 8.0, 2.5], [0, 0, 1]], np.float32)
    depth = np.full((H, W), 2.0, np.float32)
    depth[3, 4] = 0.75      # the pixel of point (1, 1, 0) at z = 1: sdf = -0.25 = -trunc, kept, t = -1
    depth[3, 0] = 1.125     # the pixel of point (0, 1, 0): u = 8 * -0.5 + 3.5 = -0.5, floor(u + 0.5) = 0: the left border is inside
    view = dict(depth=depth, w2c=np.eye(4, dtype=np.float32), k=k, image=np.full((3, H, W), 0.5, np.float32),
                labels=np.full((H, W), 123456, np.int64))
    for odd in (False, True):
        got = _integrate(vol, view, odd)
        want = _ref_integrate(vol.copy(), view).state()
        _same_state(got, want, ("exact", odd))
        lin = lambda i, j, kk: (kk * 3 + j) * 3 + i
        assert got["weight"][lin(1, 1, 0)] == 1 and got["tsdf"][lin(1, 1, 0)] == -1 and got["cweight"][lin(1, 1, 0)] == 1
        assert got["best"][lin(1, 1, 0)] == 0.25 and got["label"][lin(1, 1, 0)] == 123456
        assert got["weight"][lin(0, 1, 0)] == 1 and got["tsdf"][lin(0, 1, 0)] == 0.5 and got["cweight"][lin(0, 1, 0)] == 1
        assert got["weight"][lin(2, 1, 0)] == 0      # u = 7.5, floor(8.0) = 8 = W: the right border is outside
        assert got["weight"][lin(1, 0, 0)] == 0 and got["weight"][lin(1, 2, 0)] == 0      # v = -1.5 and 6.5: outside
        # z = 1.5: point (1, 1, 1) looks through the same pixel as (1, 1, 0): sdf = -0.75 < -trunc, skipped; point (0, 1, 1) has
        # u = 8 * (-0.5 / 1.5) + 3.5, pixel 1, depth 2: sdf = 0.5 > trunc, t = 1, outside the band
        assert got["weight"][lin(1, 1, 1)] == 0 and got["tsdf"][lin(1, 1, 1)] == 1
        assert got["weight"][lin(0, 1, 1)] == 1 and got["tsdf"][lin(0, 1, 1)] == 1 and got["cweight"][lin(0, 1, 1)] == 0


# ---- the surface ------------------------------------------------------------------------------------------------------------------------------
def _check_surface(vol, what):
    want_pos, want_faces, want_rgb, want_labels, want_keys = R.extract(vol)
    first = None
    for odd in (False, True):
        counts, keys, vkeys, faces, pos, rgb, labels = _surface(vol, odd)
        assert np.array_equal(counts, R.cube_counts(vol.X, vol.Y, vol.Z, vol.tsdf, vol.weight)), what
        assert np.array_equal(vkeys, want_keys), what
        assert np.array_equal(R.canonical_faces(faces), R.canonical_faces(want_faces)), what
        assert R.same_floats(pos, want_pos), (what, np.argwhere(pos.view(np.uint32) != want_pos.view(np.uint32))[:5])
        assert (rgb is None and want_rgb is None) or np.array_equal(rgb, want_rgb), what
        assert (labels is None and want_labels is None) or np.array_equal(labels, want_labels), what
        # emission order: cubes in linear order — the rows of cube lin follow those of every cube before it, and each of their keys
        # starts at one of that cube's corners
        cube = np.repeat(np.arange(vol.N, dtype=np.int64), counts)
        corners = np.array([R._corner_lin(0, c, vol.X, vol.Y) for c in range(8)], np.int64)
        assert len(cube) == len(keys) and np.isin((keys >> 3) - cube[:, None], corners).all(), what
        if first is None:
            first = (keys, faces, pos)
        else:      # a second run, at other addresses: identical tensors
            assert np.array_equal(first[0], keys) and np.array_equal(first[1], faces) and np.array_equal(first[2].view(np.uint32), pos.view(np.uint32))
    return first[1], first[2]


@pytest.mark.parametrize("dims", GRIDS)
def test_surface_of_the_integrated_volumes(dims):
    for W, H in IMAGES:
        vol = _fused.get((dims, W, H))
        if vol is None:      # run alone: fuse here
            vol = _volume(dims, 2.0, True, True)
            for view in _views(dims, W, H, True, True, 1000 * dims[0] + 10 * dims[1] + W):
                _ref_integrate(vol, view)
        faces, _pos = _check_surface(vol, (dims, W, H))
        if dims[0] >= 17:
            assert len(faces) > 0


def test_surface_of_a_random_volume_with_unobserved_points():
    g = np.random.default_rng(3)
    for colour, labels in MODES:
        vol = R.Volume((0.3, -0.2, 0.1), (17, 13, 11), 0.05, 0.2, 64.0, color=colour, labels=labels)
        vol.tsdf = (g.random(vol.N) * 2 - 1).astype(np.float32)
        vol.tsdf[::13] = 0.0                                        # an exact zero is outside
        vol.tsdf[5::17] = -0.0
        vol.weight = np.where(g.random(vol.N) < 0.1, 0, g.integers(1, 5, vol.N)).astype(np.float32)
        if colour:
            vol.color = (g.random((3, vol.N)) * 1.5 - 0.25).astype(np.float32)      # beyond [0, 1]: clamped
            vol.cweight = np.where(g.random(vol.N) < 0.4, 0, 1).astype(np.float32)
        if labels:
            vol.label = g.integers(-1, 100000, vol.N).astype(np.int32)
        faces, _pos = _check_surface(vol, ("random", colour, labels))
        assert len(faces) > 1000


def test_sphere_on_the_device_is_closed_manifold_and_near_the_sphere():
    vol = R.sphere_volume(TC.SPHERE_DIMS, TC.SPHERE_H, TC.SPHERE_C, TC.SPHERE_R, TC.SPHERE_TRUNC, color=True, labels=True)
    vol.color[:] = 0.25
    vol.cweight[:] = 1
    vol.label[:] = np.arange(vol.N, dtype=np.int32)
    faces, pos = _check_surface(vol, "sphere")
    TC.check_sphere_mesh(pos, faces)      # topology and distance on the DEVICE's mesh


def test_volume_object_equals_the_raw_calls():
    """hsr_utils.mesh.TsdfVolume: integrate and extract are those launches; an empty volume gives empty tensors of the right shapes"""
    from hsr_utils import mesh
    dims, W, H = (17, 13, 11), 40, 30
    ref = _volume(dims, 64.0, True, True)
    vol = mesh.TsdfVolume(ref.origin, dims, float(ref.h), trunc=float(ref.trunc), labels=True)
    assert vol.tsdf.shape == (11, 13, 17) and vol.color.shape == (3, 11, 13, 17) and vol.label.dtype == torch.int32
    assert float(vol.tsdf.min()) == 1 and not vol.weight.any() and torch.isinf(vol.best).all() and (vol.label == -1).all()
    empty = vol.extract()
    assert [tuple(t.shape) for t in empty] == [(0, 3), (0, 3), (0, 3), (0,)]
    assert [t.dtype for t in empty] == [torch.float32, torch.int32, torch.uint8, torch.int32] and all(t.is_cuda for t in empty)
    for view in _views(dims, W, H, True, True, 77):
        _ref_integrate(ref, view)
        dev = {n: torch.from_numpy(v).cuda() for n, v in view.items() if isinstance(v, np.ndarray) and n not in ("w2c", "k")}
        labels = dev["labels"].to(torch.int32) if "opacity" in view else dev["labels"]      # int32 planes are taken too
        vol.integrate(dev["depth"][None], view["w2c"], view["k"], color=dev["image"], labels=labels, opacity=dev.get("opacity"),
                      sil_thres=view.get("sil_thres"), depth_max=view.get("depth_max", 0.0))
    got = {n: getattr(vol, n).cpu().numpy().reshape(ref.state()[n].shape) for n in STATE}
    _same_state(got, ref.state(), "TsdfVolume")
    vertices, faces, rgb, labels = vol.extract()
    _counts, _keys, _vkeys, want_faces, want_pos, want_rgb, want_labels = _surface(ref)
    assert len(want_faces) > 0 and np.array_equal(faces.cpu().numpy(), want_faces) and faces.dtype == torch.int32
    assert R.same_floats(vertices.cpu().numpy(), want_pos) and np.array_equal(rgb.cpu().numpy(), want_rgb)
    assert np.array_equal(labels.cpu().numpy(), want_labels)
    again = vol.extract()
    assert all(torch.equal(a.view(torch.uint8) if a.dtype == torch.float32 else a, b.view(torch.uint8) if b.dtype == torch.float32 else b)
               for a, b in zip((vertices, faces, rgb, labels), again))
    plain = mesh.TsdfVolume(ref.origin, dims, float(ref.h), color=False)
    plain.tsdf.copy_(vol.tsdf); plain.weight.copy_(vol.weight)
    v2, f2, rgb2, lab2 = plain.extract()
    assert rgb2 is None and lab2 is None and torch.equal(f2, faces) and torch.equal(v2.view(torch.int32), vertices.view(torch.int32))
    with pytest.raises(RuntimeError, match="needs a volume made with color=True"):
        plain.integrate(dev["depth"], view["w2c"], view["k"], color=dev["image"])
    with pytest.raises(RuntimeError, match="needs a volume made with labels=True"):
        plain.integrate(dev["depth"], view["w2c"], view["k"], labels=dev["labels"])
    with pytest.raises(ValueError, match="opacity and sil_thres come together"):
        plain.integrate(dev["depth"], view["w2c"], view["k"], opacity=dev["depth"])
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        plain.integrate(dev["depth"].cpu(), view["w2c"], view["k"])


# ---- refusals on the device: the error, and every output still poisoned ------------------------------------------------------------------------
def test_every_refusal_leaves_the_outputs_untouched():
    from diff_gaussian_rasterization import _abi
    dev = _device()
    N, H, W = 4 * 3 * 2, 6, 8
    f = lambda n, v=POISON: torch.full((n,), v, dtype=torch.float32, device=dev)
    state = dict(tsdf=f(N), weight=f(N), color=f(3 * N), cweight=f(N), best=f(N), label=torch.full((N,), POISON_INT, dtype=torch.int32, device=dev))
    inputs = dict(depth=f(H * W, 1.0), image=f(3 * H * W, 0.5), labels=torch.zeros(H * W, dtype=torch.int64, device=dev), opacity=f(H * W, 1.0))
    real = {n: t.data_ptr() for n, t in list(state.items()) + list(inputs.items())}

    def clean():
        torch.cuda.synchronize()
        return all(bool((t == (POISON_INT if t.dtype == torch.int32 else POISON)).all()) for t in state.values())

    for overrides, message in TC.INTEGRATE_REFUSALS:
        rc = TC.integrate_call(_abi.lib, **dict(real, **overrides))
        err = _abi.lib.hsr_last_error()
        assert rc == -1 and err.startswith(b"tsdf_integrate: ") and message in err and clean(), (overrides, rc, err)
    # the surface entry points: real inputs, poisoned outputs
    tsdf, weight = f(N, -0.5), f(N, 1.0)
    tsdf[::2] = 0.5
    outs = dict(out_counts=torch.full((N,), POISON_INT, dtype=torch.int32, device=dev), out_keys=torch.full((3 * 12 * N,), POISON_INT, dtype=torch.int64, device=dev),
                out_vertices=f(15), out_rgb=torch.full((15,), 0xA5, dtype=torch.uint8, device=dev), out_labels=torch.full((5,), POISON_INT, dtype=torch.int32, device=dev))
    ins = dict(tsdf=tsdf, weight=weight, offsets=torch.full((N,), 5, dtype=torch.int64, device=dev), keys=torch.full((5,), 9, dtype=torch.int64, device=dev),
               color=f(3 * N, 0.5), cweight=f(N, 1.0), label=torch.zeros(N, dtype=torch.int32, device=dev))
    real = {n: t.data_ptr() for n, t in list(outs.items()) + list(ins.items())}
    for call, prefix, overrides, message in TC.SURFACE_REFUSALS:
        names = call.__code__.co_varnames[:call.__code__.co_argcount]
        rc = call(_abi.lib, **dict({n: p for n, p in real.items() if n in names}, **overrides))
        err = _abi.lib.hsr_last_error()
        torch.cuda.synchronize()
        untouched = all(bool((t == (0xA5 if t.dtype == torch.uint8 else POISON_INT if t.dtype != torch.float32 else POISON)).all()) for t in outs.values())
        assert rc == -1 and err.startswith(prefix) and message in err and untouched, (overrides, rc, err)
    # and the same calls without the overrides do write
    assert TC.integrate_call(_abi.lib, **{n: t.data_ptr() for n, t in list(state.items()) + list(inputs.items())}) == 0
    assert not clean()
    assert TC.count_call(_abi.lib, tsdf=real["tsdf"], weight=real["weight"], out_counts=real["out_counts"]) == 0
    torch.cuda.synchronize()
    assert (outs["out_counts"] >= 0).all()
