"""numpy restatement of include/ext/hsr_map_export.h, rule by rule (body_sh, body_rgb8 with colours_labels / colours_tree, tree_labels),
the header map_io.write_ply writes (header), a literal restatement of the reference's transfer_eachlevel_1 with its colour lookup
(scripts/export_ply_semantic_tree.py:183-199, :350-352), and the input lists the map-export suites build their maps from.  Host only;
tests/test_map_export_cpu.py ties the restatement to the host writers hsr_utils.map_io.save_ply / save_ply_semantic byte for byte,
tests/test_gpu_map_export.py compares the kernel against it, bit for bit."""
import numpy as np
import torch

import export_ref as X

C0F = np.float32(0.28209479177387814)
assert C0F.view(np.uint32) == 0x3e906ebb
SH_BYTES, RGB8_BYTES = 68, 59
GEOMETRY = [("float", n) for n in ("x", "y", "z", "nx", "ny", "nz")]
REST = [("float", n) for n in ("opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3")]
FIELDS_SH = GEOMETRY + [("float", n) for n in ("f_dc_0", "f_dc_1", "f_dc_2")] + REST
FIELDS_RGB8 = GEOMETRY + [("uchar", n) for n in ("red", "green", "blue")] + REST
COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)      # Gaussians: around a wave, around a workgroup, three workgroups and a tail

NAN_PAYLOAD = np.array([0x7fc12345, 0xffc00001, 0x7f800001], dtype=np.uint32).view(np.float32)      # two quiet NaNs, one signalling


def rgb_values():
    """float32: 0, 0.5, 1, the floats either side of 0.5, denormals, the infinities, a NaN, values outside 0..1 and plain fractions"""
    half = np.float32(0.5)
    return np.array([0.0, 0.5, 1.0, np.nextafter(half, np.float32(0)), np.nextafter(half, np.float32(1)), 1e-40, -1e-40, 1.4e-45,
                     np.inf, -np.inf, np.nan, -0.0, 2.0, -1.0, 0.25, 0.75, 0.1, 0.9, 0.33333334, 3e38], dtype=np.float32)


def make_map(P, S, K, seed):
    """a map of P Gaussians as float32 numpy arrays (logit_opacities [P,1], log_scales [P,S], semantic [P,K]): random values with the
    rgb list above laid over rgb_colors, NaNs of three payloads, an infinity and a denormal in the copied arrays, and logits on a grid
    of 1/64 (so that the values of a level are equal or apart by at least 1/64: export_ref.level_labels' condition)"""
    g = np.random.default_rng(seed)
    m = {"means3D": g.normal(size=(P, 3)), "rgb_colors": g.random(size=(P, 3)), "unnorm_rotations": g.normal(size=(P, 4)),
         "logit_opacities": g.normal(size=(P, 1)) * 3, "log_scales": g.normal(size=(P, S)) - 4, "normals": g.normal(size=(P, 3))}
    m = {k: v.astype(np.float32) for k, v in m.items()}
    random_rgb = m["rgb_colors"]
    m["rgb_colors"] = X.lay(rgb_values(), (P, 3), shift=seed % 20)      # every listed value once P >= 7; a small map starts anywhere
    m["rgb_colors"][7::8] = random_rgb[7::8]
    for k, name in enumerate(("means3D", "unnorm_rotations", "logit_opacities", "log_scales", "normals")):
        flat = m[name].reshape(-1)
        special = np.concatenate([NAN_PAYLOAD, np.array([np.inf, -np.inf, 1e-40, -0.0], dtype=np.float32)])
        if flat.size:
            flat[(np.arange(len(special)) * 5 + k) % flat.size] = special
    m["semantic"] = (g.integers(-128, 129, size=(P, K)) / 64.0).astype(np.float32)
    return m


def assert_separated(x, sizes):
    """the condition under which export_ref.level_labels is the header's label: finite values, within a level equal or apart by more than
    1e-6 (checked on the host before any use of the restatement).  x: float32 [P,K]"""
    begin = 0
    for s in sizes:
        level = np.sort(x[:, begin:begin + s].astype(np.float64), axis=1)
        assert np.isfinite(level).all()
        gaps = np.diff(level, axis=1)
        assert ((gaps == 0) | (gaps > 1e-6)).all()
        begin += s


def tree_labels(x, sizes):
    """float32 [P,K] -> int64 [L,P]: the header's per-level labels, through export_ref.level_labels on the transposed logits"""
    assert x.dtype == np.float32 and x.ndim == 2
    assert_separated(x, sizes)
    return X.level_labels(np.ascontiguousarray(x.T)[:, None, :], sizes)[:, 0, :]


def colours_labels(labels, table):
    """int32 [P], uint8 [n,3] -> uint8 [P,3]: table[label] inside the table, black outside (no wrap of negative labels)"""
    return X.labels(labels.reshape(1, -1), table)[0]


def colours_tree(x, sizes, table):
    """float32 [P,K] -> uint8 [P,3]: the tuple table at the mixed-radix index of the level labels, level 0 most significant"""
    return X.levels(tree_labels(x, sizes)[:, None, :], sizes, table)[0]


def _bits(a, cols):
    a = np.ascontiguousarray(a, dtype="<f4")
    assert a.shape[1] == cols
    return a.view(np.uint8).reshape(a.shape[0], 4 * cols)


def _scales3(scales):
    return np.tile(scales, (1, 3)) if scales.shape[1] == 1 else scales      # np.tile, :259-260


def f_dc(rgb):
    """one fp32 subtraction, one correctly rounded fp32 division by the fp32 nearest to C0"""
    assert rgb.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        out = (rgb - np.float32(0.5)) / C0F
    assert out.dtype == np.float32
    return out


def body_sh(m, normals=None):
    """uint8 [P,68]: x y z  nx ny nz  f_dc_0..2  opacity  scale_0..2  rot_0..3, every float but f_dc a bit copy"""
    P = m["means3D"].shape[0]
    normals = np.zeros((P, 3), dtype=np.float32) if normals is None else normals
    rec = np.concatenate([_bits(m["means3D"], 3), _bits(normals, 3), _bits(f_dc(m["rgb_colors"]), 3), _bits(m["logit_opacities"].reshape(P, 1), 1),
                          _bits(_scales3(m["log_scales"]), 3), _bits(m["unnorm_rotations"], 4)], axis=1)
    assert rec.shape == (P, SH_BYTES)
    return rec


def body_rgb8(m, colours, normals=None):
    """uint8 [P,59]: the same with red green blue as bytes at offset 24"""
    P = m["means3D"].shape[0]
    normals = np.zeros((P, 3), dtype=np.float32) if normals is None else normals
    assert colours.dtype == np.uint8 and colours.shape == (P, 3)
    rec = np.concatenate([_bits(m["means3D"], 3), _bits(normals, 3), colours, _bits(m["logit_opacities"].reshape(P, 1), 1),
                          _bits(_scales3(m["log_scales"]), 3), _bits(m["unnorm_rotations"], 4)], axis=1)
    assert rec.shape == (P, RGB8_BYTES)
    return rec


def header(count, fields):
    lines = ["ply", "format binary_little_endian 1.0", "element vertex %d" % count]
    lines += ["property %s %s" % (kind, name) for kind, name in fields]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def same_body(got, want, stride):
    """got (uint8, flat) equals want (uint8 [P,stride]) byte for byte; in 68-byte records a NaN f_dc of the restatement asks for a NaN,
    whatever its payload"""
    got = np.asarray(got)
    assert got.dtype == np.uint8 and got.size == want.size, (got.size, want.size)
    got = got.reshape(want.shape).copy()
    want = want.copy()
    if stride == SH_BYTES:
        gf, wf = got[:, 24:36].copy().view("<f4"), want[:, 24:36].copy().view("<f4")
        nan = np.isnan(wf)
        assert np.isnan(gf[nan]).all() and not np.isnan(gf[~nan]).any()
        mask = np.repeat(nan, 4, axis=1)
        got[:, 24:36][mask] = 0
        want[:, 24:36][mask] = 0
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)[0]
        raise AssertionError("record %d byte %d: got %d, want %d" % (bad[0], bad[1], got[bad[0], bad[1]], want[bad[0], bad[1]]))


# ---- the reference's lines, literally ------------------------------------------------------------------------------------------------
def eachlevel_literal(levels, idx_mapping):
    """transfer_eachlevel_1 (:183-199): levels int64 tensor [l,P]; idx_mapping the dict of the level; returns (labels [P] with -1 where
    no key matched, the dict's length)"""
    label = torch.full((levels.shape[1], 1), -1)
    for idx, (key, _value) in enumerate(idx_mapping.items(), start=0):
        key = torch.tensor(key).unsqueeze(1)
        index = torch.all(levels == key, dim=0)
        label[index] = idx
    return label.squeeze(1), len(idx_mapping)


def multilevel_colours_literal(levels, idx_mapping, label_colormap):
    """:350-352 with the one stated difference: label_colormap(num_dim)[label], and BLACK where the label stayed -1 (numpy would wrap it
    to the last colour).  label_colormap: n -> uint8 [n,3] numpy"""
    label, num_dim = eachlevel_literal(levels, idx_mapping)
    label = label.numpy()
    colours = label_colormap(num_dim)[label]
    colours[label < 0] = 0
    return colours
