"""GPU suite for hsr_keyframe_pack / hsr_keyframe_unpack and hsr_utils.checkpoint.pack_keyframe / unpack_keyframe: the codes and the three
counters EQUAL to the numpy restatement (tests/keyframe_pack_ref.py), no tolerance.

Sizes by pixel count N, where the kernel can go wrong: the 4-value vector tail (1, 3x5 = 15, 37x53 = 1961 = 1 mod 4), planes that
start off 16 bytes (every N that is no multiple of 4, from the second plane on), the 1024-value workgroup edge (1x1023, 32x32 = 1024,
25x41 = 1025) and several workgroups (96x128 = 12 of them); with L in {0, 1, 5, 17} label planes, colour or depth absent, base
pointers one element off (the one-value path), planted defects at the first value, the last one and in the vector tail, and one
keyframe of the flagship size."""
import numpy as np
import pytest
import torch

import keyframe_pack_ref as R

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 5), (37, 53), (1, 1023), (32, 32), (25, 41), (96, 128)]
PLANES = [0, 1, 5, 17]
SCALES = [6553.5, 1000.0, 5000.0]


def _exact_planes(H, W, L, scale, seed):
    """planes built from random 8-/16-bit codes through the ingest expressions: what ingest() at sensor size gives"""
    rng = np.random.default_rng(seed)
    color = R.ingest_colour(rng.integers(0, 256, (3, H, W)).astype(np.float32))
    depth = R.ingest_depth(rng.integers(0, 65536, (H, W)).astype(np.float64), scale)
    labels = rng.integers(0, 65536, (L, H, W)).astype(np.int64) if L else None
    return color, depth, labels


def _dev(a, off=0):
    """the array on the device; off = 1: as a view one element into a larger allocation, so that its base pointer is off the vector alignment"""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not off:
        return t.cuda()
    flat = torch.empty(t.numel() + off, dtype=t.dtype, device="cuda")
    view = flat[off:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 or t.element_size() < 4
    return view


def _empty(shape, dtype, off=0):
    n = int(np.prod(shape))
    flat = torch.full((n + off,), 0x55, dtype=dtype, device="cuda")
    return flat[off:].view(shape)


def _pack(color, depth, labels, scale, off=0):
    """hsr_keyframe_pack on numpy planes (None: the group is absent) -> (colour codes, depth codes, label codes, lossy) as numpy"""
    from diff_gaussian_rasterization import _abi
    ref = next(a for a in (color, depth, labels) if a is not None)
    H, W = ref.shape[-2:]
    L = 0 if labels is None else labels.shape[0]
    c, d, lab = _dev(color, off), _dev(depth, off), _dev(labels, off)
    oc = None if c is None else _empty((3, H, W), torch.uint8, off)
    od = None if d is None else _empty((H, W), torch.int16, off)
    ol = None if lab is None else _empty((L, H, W), torch.int16, off)
    lossy = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    scratch = torch.full((int(_abi.lib.hsr_keyframe_pack_scratch_bytes(H, W, L)),), 0xAB, dtype=torch.uint8, device="cuda")      # never cleared
    dev = torch.device("cuda", torch.cuda.current_device())

    def p(t):
        return None if t is None else t.data_ptr()
    _abi.call(_abi.lib.hsr_keyframe_pack, "hsr_keyframe_pack", dev, H, W, p(c), p(d), L, p(lab), scale, p(oc), p(od), p(ol), lossy.data_ptr(),
              scratch.data_ptr(), scratch.numel())

    def host(t, view=None):
        return None if t is None else (t.cpu().numpy() if view is None else t.cpu().numpy().view(view))
    return host(oc), host(od, np.uint16), host(ol, np.uint16), lossy.cpu().numpy().view(np.uint32)


def _unpack(c8, d16, l16, scale, off=0):
    from diff_gaussian_rasterization import _abi
    ref = next(a for a in (c8, d16, l16) if a is not None)
    H, W = ref.shape[-2:]
    L = 0 if l16 is None else l16.shape[0]
    c, d, lab = _dev(c8, off), _dev(None if d16 is None else d16.view(np.int16), off), _dev(None if l16 is None else l16.view(np.int16), off)
    oc = None if c is None else _empty((3, H, W), torch.float32, off)
    od = None if d is None else _empty((H, W), torch.float32, off)
    ol = None if lab is None else _empty((L, H, W), torch.int64, off)
    dev = torch.device("cuda", torch.cuda.current_device())

    def p(t):
        return None if t is None else t.data_ptr()
    _abi.call(_abi.lib.hsr_keyframe_unpack, "hsr_keyframe_unpack", dev, H, W, p(c), p(d), L, p(lab), scale, p(oc), p(od), p(ol))
    return tuple(None if t is None else t.cpu().numpy() for t in (oc, od, ol))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.int64 else a.dtype)


def _check(color, depth, labels, scale, off=0):
    """pack equals the restatement (codes and counters), and unpacking the codes equals the restatement's unpack; returns (codes, lossy, unpacked)"""
    want = R.pack(color, depth, labels, scale)
    got = _pack(color, depth, labels, scale, off)
    for name, w, g in zip(("colour", "depth", "labels"), want[:3], got[:3]):
        assert (w is None) == (g is None), name
        if w is not None:
            assert g.dtype == w.dtype and np.array_equal(g, w), (name, int((g != w).sum()))
    assert got[3].tolist() == want[3].tolist(), (got[3], want[3])
    back = _unpack(got[0], got[1], got[2], scale, off)
    for name, w, g in zip(("colour", "depth", "labels"), R.unpack(want[0], want[1], want[2], scale), back):
        if w is not None:
            assert g.dtype == w.dtype and np.array_equal(_bits(g), _bits(w)), name
    return got[:3], got[3], back


@pytest.mark.parametrize("L", PLANES)
@pytest.mark.parametrize("H,W", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_exact_planes_pack_with_zero_counters_and_come_back_bit_for_bit(H, W, L):
    scale = SCALES[(H + L) % 3]
    color, depth, labels = _exact_planes(H, W, L, scale, seed=H * 131 + W * 7 + L)
    _codes, lossy, back = _check(color, depth, labels, scale)
    assert lossy.tolist() == [0, 0, 0]
    assert np.array_equal(_bits(back[0]), _bits(color)) and np.array_equal(_bits(back[1]), _bits(depth))
    assert (labels is None and back[2] is None) or np.array_equal(back[2], labels)


@pytest.mark.parametrize("absent", ["color", "depth", "both"])
@pytest.mark.parametrize("H,W", [(37, 53), (25, 41)], ids=["37x53", "25x41"])
def test_absent_groups(H, W, absent):
    color, depth, labels = _exact_planes(H, W, 5, 1000.0, seed=5)
    depth[0, 0] = np.float32(0.5e-3)      # between two codes: counted only when the depth is there
    color[2, -1, -1] = np.float32(0.3)
    c = None if absent in ("color", "both") else color
    d = None if absent in ("depth", "both") else depth
    _codes, lossy, _back = _check(c, d, labels, 1000.0)
    assert lossy.tolist() == [0 if c is None else 1, 0 if d is None else 1, 0]
    if absent != "both":
        _check(c, d, None, 1000.0)      # and without labels: L = 0


@pytest.mark.parametrize("L", [0, 5])
@pytest.mark.parametrize("H,W", [(3, 5), (37, 53), (32, 32), (25, 41)], ids=["3x5", "37x53", "32x32", "25x41"])
def test_base_pointers_one_element_off_take_the_one_value_path(H, W, L):
    color, depth, labels = _exact_planes(H, W, L, 6553.5, seed=9)
    color[1, H // 2, W // 2] = np.float32("nan")
    _codes, lossy, _back = _check(color, depth, labels, 6553.5, off=1)
    assert lossy.tolist() == [1, 0, 0]


def _plant(plane, places, values):
    flat = plane.reshape(-1)
    for at, v in zip(places, values):
        flat[at] = v
    return set(places)


@pytest.mark.parametrize("H,W", [(37, 53), (25, 41), (96, 128)], ids=["37x53", "25x41", "96x128"])
def test_planted_defects_are_counted_and_everything_else_comes_back(H, W):
    scale, L, N = 6553.5, 5, H * W
    color, depth, labels = _exact_planes(H, W, L, scale, seed=21)
    tail = N - 1 if N % 4 else N - 2      # a value of the last, partial quad where there is one
    # colour: first value, last value of the frame's last plane, the tail of plane 0, and two in the middle of plane 1
    bad_c = _plant(color, [0, 3 * N - 1, tail, N + 7, N + N // 2],
                   [np.float32("nan"), np.float32("inf"), np.float32(-0.0), np.float32(1.0000001), np.float32(-1e-9)])
    between = np.float32((np.float64(R.ingest_depth(100, scale)) + np.float64(R.ingest_depth(101, scale))) / 2)
    bad_d = _plant(depth, [0, N - 1, tail - 1 if tail - 1 > 0 else 1, N // 2, N // 3],
                   [between, np.float32(65536.5 / scale), np.float32("nan"), np.float32("-inf"), np.float32(-0.0)])
    bad_l = _plant(labels, [0, L * N - 1, tail], [-1, 65536, -2 ** 40])
    labels.reshape(-1)[[1, N, 2 * N + 5]] = 65535      # the largest code: fine
    codes, lossy, back = _check(color, depth, labels, scale)
    assert lossy.tolist() == [len(bad_c), len(bad_d), len(bad_l)] == [5, 5, 3]
    assert codes[0].reshape(-1)[[0, 3 * N - 1, tail, N + 7, N + N // 2]].tolist() == [0, 255, 0, 255, 0]      # an inexact value writes its clamped code
    assert codes[1].reshape(-1)[[N - 1, N // 2]].tolist() == [65535, 0] and codes[2].reshape(-1)[[0, L * N - 1, tail]].tolist() == [0, 65535, 0]
    for plane, bad, out in ((color, bad_c, back[0]), (depth, bad_d, back[1]), (labels, bad_l, back[2])):
        keep = np.ones(plane.size, bool)
        keep[sorted(bad)] = False
        assert np.array_equal(_bits(out).reshape(-1)[keep], _bits(plane).reshape(-1)[keep])
        assert not np.array_equal(_bits(out).reshape(-1)[~keep], _bits(plane).reshape(-1)[~keep])


def test_a_keyframe_of_the_flagship_size():
    H, W, L, scale = 680, 1200, 5, 6553.5
    color, depth, labels = _exact_planes(H, W, L, scale, seed=3)
    color[0, 0, 0], depth[-1, -1], labels[4, -1, -1] = np.float32(0.123), np.float32(3.0000001), -1
    _codes, lossy, _back = _check(color, depth, labels, scale)
    assert lossy.tolist() == [1, 1, 1]


# ---- pack_keyframe / unpack_keyframe: always exact, whatever came in -------------------------------------------------------------------------
def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))


@pytest.mark.parametrize("kind", ["exact", "bilinear colour", "inexact", "no scale", "no labels"])
def test_pack_keyframe_round_trip_is_bit_exact(kind):
    from hsr_utils import pack_keyframe, unpack_keyframe
    H, W, scale = 37, 53, 6553.5
    color, depth, labels = (torch.from_numpy(a).cuda() for a in _exact_planes(H, W, 3, scale, seed=31))
    depth = depth[None]
    want = {"color": True, "depth": True, "labels": True}
    if kind in ("bilinear colour", "inexact"):      # an 8-bit image resized: no longer a grey level over 255
        big = torch.from_numpy(R.ingest_colour(np.random.default_rng(1).integers(0, 256, (3, 2 * H + 1, 2 * W + 3)).astype(np.float32))).cuda()
        color = torch.nn.functional.interpolate(big[None], size=(H, W), mode="bilinear", align_corners=False)[0].contiguous()
        want["color"] = False
    if kind == "inexact":
        depth = torch.rand(1, H, W, device="cuda") * 5
        labels = labels - 40000
        want["depth"] = want["labels"] = False
    if kind == "no scale":
        scale, want["depth"] = None, False
    if kind == "no labels":
        labels = None
        del want["labels"]
    pk = pack_keyframe(color, depth, labels, depth_scale=scale)
    assert pk.exact == want
    assert set(pk.codes) == {g for g, e in want.items() if e} and set(pk.raw) == {g for g, e in want.items() if not e}
    counts = pk.lossy_counts
    assert [c == 0 for c in counts[:2]] == [want["color"], want["depth"] or scale is None] and (counts[2] == 0) == want.get("labels", True)
    c, d, lab = unpack_keyframe(pk)
    assert _same(c, color) and _same(d, depth) and d.shape == (1, H, W)
    assert (lab is None and labels is None) or _same(lab, labels)
    if kind == "exact":
        assert pk.nbytes() == H * W * (3 + 2 + 2 * 3)
