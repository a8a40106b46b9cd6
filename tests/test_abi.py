"""CPU suite: the C-ABI library loads and exports exactly what include/hsr_*.h and include/ext/*.h declare, the ctypes signatures,
structures and limits of diff_gaussian_rasterization/_abi.py agree with the headers type class by type class, and host-only entry
points behave (no compute calls: there is no GPU here).  A header is named by its path under include/, the key of _abi.HEADERS."""
import ctypes as C
import glob
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
# globs: the next header is covered without an edit
HEADERS = sorted(os.path.relpath(p, INCLUDE) for p in glob.glob(os.path.join(INCLUDE, "hsr_*.h")))
ALL_HEADERS = HEADERS + sorted(os.path.relpath(p, INCLUDE).replace(os.sep, "/") for p in glob.glob(os.path.join(INCLUDE, "ext", "*.h")))
# asserted as numbers: a regex that silently stops matching must not pass
PROTOTYPE_COUNTS = {
    "hsr_rasterizer.h": 24, "hsr_frame_prep.h": 4, "hsr_losses.h": 14, "hsr_densify.h": 5, "hsr_eval.h": 9, "hsr_optim.h": 3,
    "hsr_keyframes.h": 5,
    "ext/hsr_msssim.h": 2, "ext/hsr_map_init.h": 2, "ext/hsr_frame_resample.h": 1, "ext/hsr_loss_outlier.h": 4,
    "ext/hsr_frame_ingest.h": 1, "ext/hsr_frame_export.h": 1, "ext/hsr_frame_ingest_planes.h": 1, "ext/hsr_map_export.h": 1,
    "ext/hsr_view.h": 3, "ext/hsr_replay.h": 5, "ext/hsr_keyframe_pack.h": 3, "ext/hsr_tsdf.h": 4,
}
N_PROTOTYPES = 64      # those of include/hsr_*.h
N_ALL_PROTOTYPES = 92

# what the four older headers declare at least (the newer ones are pinned by name, each in its own suite: test_eval_cpu.py,
# test_optim_cpu.py, test_keyframes_cpu.py and the suites of the headers under include/ext/)
DECLARED = {
    "hsr_rasterizer.h": {
        "hsr_forward", "hsr_forward_semantic", "hsr_backward", "hsr_backward_semantic", "hsr_mark_visible", "hsr_required_geometry_bytes",
        "hsr_required_image_bytes", "hsr_required_binning_bytes", "hsr_last_error", "hsr_version", "hsr_get_state_layout",
        "hsr_profile_enable", "hsr_profile_read", "hsr_stage_name"},
    "hsr_frame_prep.h": {"hsr_frame_prep_forward", "hsr_frame_prep_backward", "hsr_frame_prep_backward_params",
                         "hsr_frame_prep_scratch_bytes"},
    "hsr_losses.h": {
        "hsr_loss_l1", "hsr_loss_l1_grad", "hsr_loss_ssim", "hsr_loss_ssim_value", "hsr_loss_ssim_grad", "hsr_loss_tree_ce",
        "hsr_loss_tree_ce_value", "hsr_loss_tree_ce_grad", "hsr_loss_tree_ce_scratch_bytes", "hsr_loss_tracking_value",
        "hsr_loss_tracking_grad", "hsr_loss_tracking_scratch_bytes", "hsr_loss_leaf_mlp_ce", "hsr_loss_scratch_bytes"},
    "hsr_densify.h": {"hsr_densify_frame", "hsr_densify_scratch_bytes", "hsr_prune_mask", "hsr_compact_append_rows",
                      "hsr_compact_scratch_bytes"},
}
SCALARS = {"int": "int", "unsigned": "unsigned", "float": "float", "double": "double", "size_t": "size_t"}


def _source(header):
    """a header's text without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)


def _classify(decl, named):
    """the class of one C parameter (`named`: the declaration ends in the parameter's name) or return type: one of SCALARS,
    "const char*" (a return type only; as a parameter it is a device pointer like any other), or ("pointer", pointee type)"""
    words = decl.replace("*", " * ").split()
    if named:
        assert re.fullmatch(r"\w+", words[-1]), decl
        words = words[:-1]
    if "*" in words:
        assert words.count("*") == 1 and words[-1] == "*", decl
        pointee = [w for w in words[:-1] if w != "const"]
        assert len(pointee) == 1, decl
        return "const char*" if (not named and words == ["const", "char", "*"]) else ("pointer", pointee[0])
    assert len(words) == 1 and words[0] in SCALARS, "unparsed C type: %r" % decl
    return SCALARS[words[0]]


def _prototypes(headers=HEADERS):
    """every function prototype of the given headers, in their order: name -> (header, class of the return type, [class of each
    parameter])"""
    protos = {}
    for header in headers:
        for m in re.finditer(r"^((?:const\s+)?\w+\s*\*?)\s*(hsr_\w+)\s*\(([^;{}()]*)\)\s*;", _source(header), flags=re.M):
            ret, name, params = m.group(1), m.group(2), m.group(3).strip()
            assert name not in protos, name
            params = [] if params in ("", "void") else [_classify(p, True) for p in params.split(",")]
            protos[name] = (header, _classify(ret, False), params)
    return protos


def _structures(headers=ALL_HEADERS):
    """every `typedef struct` of the given headers: name -> [field names in order]; an array member `int sizes[16]` is `sizes`"""
    structs = {}
    for header in headers:
        for m in re.finditer(r"typedef struct (hsr_\w+) \{(.*?)\} \1;", _source(header), flags=re.S):
            assert m.group(1) not in structs, m.group(1)
            structs[m.group(1)] = [re.search(r"(\w+)\s*(?:\[\w+\])?\s*$", d).group(1)
                                   for stmt in m.group(2).split(";") if stmt.strip() for d in stmt.split(",")]
    return structs


def _ctype_class(t):
    """the class of a ctypes type, in the vocabulary of _classify; a pointer names its pointee where ctypes knows it"""
    for ct, cls in ((C.c_int, "int"), (C.c_uint, "unsigned"), (C.c_float, "float"), (C.c_double, "double"), (C.c_size_t, "size_t"),
                    (C.c_char_p, "const char*")):
        if t is ct:
            return cls
    if t is C.c_void_p:
        return ("pointer", None)
    if isinstance(t, type) and issubclass(t, C._Pointer):
        pointee = t._type_
        return ("pointer", pointee.__name__ if issubclass(pointee, C.Structure) else _ctype_class(pointee))
    raise AssertionError("a ctypes type this test does not know: %r" % (t,))


def _agree(declared, header):
    """does a ctypes class satisfy a header class?  Scalars must be equal.  Any ctypes pointer satisfies a pointer, but one that
    names its pointee must name the header's: POINTER(struct) the same struct, POINTER(c_int) an int."""
    if isinstance(header, tuple) and isinstance(declared, tuple):
        return declared[1] is None or declared[1] == header[1]
    return declared == header


def check_signature(name, proto):
    """the declared ctypes signature of `name` agrees with its prototype (an entry of _prototypes()) class by class"""
    from diff_gaussian_rasterization import _abi
    header, ret, params = proto
    fn = getattr(_abi.lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == len(params), (name, len(fn.argtypes or ()), len(params))
    assert _agree(_ctype_class(fn.restype), ret), "%s (%s): restype %r, the header returns %r" % (name, header, fn.restype, ret)
    for i, (t, cls) in enumerate(zip(fn.argtypes, params)):
        assert _agree(_ctype_class(t), cls), "%s (%s): parameter %d (from 0) is %s, the header says %r" % (name, header, i, t.__name__, cls)


def check_header(header):
    """every prototype of include/<header> is exported by the library and bound with the header's types; returns their names in the
    header's order"""
    from diff_gaussian_rasterization import _C
    protos = _prototypes([header])
    lib = C.CDLL(_C._LIB_PATH)
    for name, proto in protos.items():
        assert hasattr(lib, name), "libhsr_rast.so does not export %s" % name
        check_signature(name, proto)
    return list(protos)


@pytest.mark.parametrize("header", ALL_HEADERS)
def test_header_is_bound_under_its_key(header):
    """the one header check: the header has a key in _abi.HEADERS whose names are its prototypes in its order (so that a line can be
    read against its prototype), as many as are pinned; the library exports each and each is bound with the header's type classes
    (int / unsigned / float / double / size_t / const char* / pointer): ctypes converts silently, so a c_int where the header says
    float would hand a kernel a wrong value and nothing else would notice"""
    from diff_gaussian_rasterization import _abi
    assert header in _abi.HEADERS, "no key %r in _abi.HEADERS" % header
    names = list(_prototypes([header]))
    assert header in PROTOTYPE_COUNTS and len(names) == PROTOTYPE_COUNTS[header], (header, len(names))
    assert [s[0] for s in _abi.HEADERS[header]] == names, header
    assert check_header(header) == names


def test_tables_cover_the_headers_and_bind_every_name_once():
    """a header without a table fails and a table without a header fails; no function name occurs twice across all tables, whichever
    two they are in"""
    from diff_gaussian_rasterization import _abi
    assert len(ALL_HEADERS) == len(set(ALL_HEADERS)) >= 19
    assert set(_abi.HEADERS) == set(ALL_HEADERS) == set(PROTOTYPE_COUNTS), set(_abi.HEADERS) ^ set(ALL_HEADERS)
    names = [s[0] for table in _abi.HEADERS.values() for s in table]
    assert sorted(names) == sorted(set(names)), sorted(n for n in set(names) if names.count(n) > 1)
    assert len(names) == len(_prototypes(ALL_HEADERS)) == sum(PROTOTYPE_COUNTS.values()) == N_ALL_PROTOTYPES


def test_library_exports_every_declared_symbol():
    from diff_gaussian_rasterization import _C
    protos = _prototypes()
    assert len(HEADERS) >= 7 and len(protos) == N_PROTOTYPES, (len(HEADERS), len(protos))
    for header, names in DECLARED.items():
        assert names <= {n for n, p in protos.items() if p[0] == header}, header
    lib = C.CDLL(_C._LIB_PATH)
    for name in protos:
        assert hasattr(lib, name), "libhsr_rast.so does not export %s" % name


def test_ctypes_signatures_match_header():
    """the tables of include/hsr_*.h taken together: every prototype once and nothing else, each header's functions in the header's
    order, every signature agreeing with its prototype class by class"""
    from diff_gaussian_rasterization import _abi
    protos = _prototypes()
    table = [s[0] for header in HEADERS for s in _abi.HEADERS[header]]
    assert sorted(table) == sorted(protos), set(table) ^ set(protos)      # every prototype once, nothing else
    for header in HEADERS:
        of_header = [n for n, p in protos.items() if p[0] == header]
        assert [n for n in table if n in of_header] == of_header, header
    for name, proto in protos.items():
        check_signature(name, proto)


def test_structures_match_header():
    """the nine ctypes structures carry the field names of their typedefs, in order; the Adam entry keeps the library's size"""
    from diff_gaussian_rasterization import _C, _abi
    from hsr_utils import optim, slam_external
    checked = set()
    for name, fields in _structures(ALL_HEADERS).items():
        mirror = getattr(_abi, name, None)
        if mirror is None:
            assert name == "hsr_profile", name      # the one typedef without a mirror
            continue
        assert fields == [f[0] for f in mirror._fields_], name
        checked.add(mirror)
    assert checked == {_abi.hsr_buffer, _abi.hsr_ticket, _abi.hsr_state_layout, _abi.hsr_adam_tensor, _abi.hsr_row_table,
                       _abi.hsr_backward_plan, _abi.hsr_ingest_level, _abi.hsr_export_job, _abi.hsr_map_export_job}
    assert (_C._HsrBuffer, _C._Ticket, _C._StateLayout) == (_abi.hsr_buffer, _abi.hsr_ticket, _abi.hsr_state_layout)
    assert optim._AdamTensor is _abi.hsr_adam_tensor and slam_external._RowTable is _abi.hsr_row_table
    assert _abi.lib.hsr_adam_table_entry_bytes() == C.sizeof(_abi.hsr_adam_tensor) == 64


def test_python_limits_equal_header_defines():
    from diff_gaussian_rasterization import _C
    from hsr_utils import evaluate, keyframes, losses, slam_external
    defines = {m.group(1): int(m.group(2)) for h in HEADERS
               for m in re.finditer(r"^#define\s+(HSR_\w+)\s+\(?(-?\d+)\)?\s*$", _source(h), flags=re.M)}
    for value, name in ((evaluate.MAX_CLASSES, "HSR_EVAL_MAX_CLASSES"), (evaluate.MAX_LEVELS, "HSR_EVAL_MAX_LEVELS"),
                        (evaluate.LEAF_MAX_K, "HSR_EVAL_LEAF_MAX_K"), (evaluate.LEAF_MAX_C, "HSR_EVAL_LEAF_MAX_C"),
                        (evaluate.MAX_DILATION, "HSR_EVAL_MAX_DILATION"), (keyframes.MAX_POINTS, "HSR_KF_MAX_POINTS"),
                        (losses.SUM, "HSR_LOSS_SUM"), (losses.MEAN, "HSR_LOSS_MEAN"), (_C.HSR_PENDING, "HSR_PENDING"),
                        (_C.HSR_ERR_BUFFER_TOO_SMALL, "HSR_ERR_BUFFER_TOO_SMALL"), (slam_external.MAX_TABLES, "HSR_MAX_ROW_TABLES")):
        assert value == defines[name], (name, value, defines[name])


def test_host_only_entry_points():
    from diff_gaussian_rasterization import _C
    lib = _C._lib
    assert b"gfx950" in lib.hsr_version()
    g1, g2 = lib.hsr_required_geometry_bytes(1000), lib.hsr_required_geometry_bytes(2000)
    assert 0 < g1 < g2
    assert lib.hsr_required_image_bytes(1200, 680) > 8 * 1200 * 680
    assert lib.hsr_required_binning_bytes(0) > 0 and lib.hsr_required_binning_bytes(10 ** 6) > 24 * 10 ** 6
    lay = _C.state_layout(1000, 64, 48, 5000)
    offs = [lay[k] for k in ("geom_depths", "geom_means2D", "geom_conic_opacity", "geom_cov3D")]
    assert offs == sorted(offs) and all(o % 256 == 0 for o in lay.values())
    for i in range(9):
        assert lib.hsr_stage_name(i) not in (None, b"?")
    assert lib.hsr_stage_name(99) == b"?"


def test_argument_validation_without_gpu():
    """invalid sizes are rejected before any device work, with a message in hsr_last_error()"""
    from diff_gaussian_rasterization import _C
    lib = _C._lib
    null = None
    rc = lib.hsr_forward_semantic(None, None, None, 10, 0, 0, 26, null, 0, 48, *([null] * 6), 1.0, *([null] * 5), 1.0, 1.0, 0,
                                  *([null] * 6), 0, null)
    assert rc == -1 and b"invalid sizes" in lib.hsr_last_error()
    rc = lib.hsr_mark_visible(-1, null, null, null, null, null)
    assert rc == -1
    from hsr_utils import slam_helpers  # sets the argtypes of the frame-prep entry points
    assert slam_helpers._lib.hsr_frame_prep_scratch_bytes(0) > 0
    assert slam_helpers._lib.hsr_frame_prep_scratch_bytes(10 ** 6) >= (10 ** 6 // 1024) * 64
    rc = lib.hsr_frame_prep_forward(10, 2, 0, 0, *([null] * 6), 1, 0, *([null] * 8))
    assert rc == -1 and b"log_scales must be" in lib.hsr_last_error()
    rc = lib.hsr_frame_prep_backward(0, 1, 0, 0, *([null] * 6), 1, 5, *([null] * 14), 0, null)
    assert rc == -1 and b"time_idx" in lib.hsr_last_error()
    from hsr_utils import losses  # sets the argtypes of the loss entry points
    assert losses._lib.hsr_loss_scratch_bytes(3, 680, 1200) >= 3 * 3 * 680 * 1200 * 4
    assert lib.hsr_loss_l1(0, 8, 8, null, null, null, 0, null, null, null, 0, null) == -1 and b"loss_l1" in lib.hsr_last_error()
    assert lib.hsr_loss_ssim(3, 0, 8, null, null, null, null, null, 0, null) == -1
    assert lib.hsr_loss_tree_ce(4, 8, 8, 1, None, None, null, null, -100, null, null, null, 0, null) == -1
    assert lib.hsr_loss_leaf_mlp_ce(40, 10, 8, 8, null, null, null, null, -100, null, null, null, null, null, 0, null) == -1
    assert b"K <= 31" in lib.hsr_last_error()
    from hsr_utils import densify  # sets the argtypes of the densification entry points
    assert densify._lib.hsr_densify_scratch_bytes(680, 1200) > 680 * 1200 // 256 * 4
    assert lib.hsr_densify_frame(0, 8, *([null] * 4), 1.0, 1.0, 0.0, 0.0, null, 0.5, 50.0, 0, *([null] * 7), null, 0, null) == -1
    # two refusals that depend on the arguments alone, in otherwise plausible calls: `d` stands for device memory and is never
    # followed.  The buffer descriptors are NULL, so a call that got as far as acquiring one would say so instead.
    dummy = C.create_string_buffer(256)
    d = C.addressof(dummy)
    rc = lib.hsr_forward(None, None, None, 10, 0, 0, d, 32, 16, d, null, d, d, d, 1.0, d, null, d, d, d, 1.0, 1.0, 0,
                         d, d, d, d, null, null, 0, null)                                        # out_mask NULL
    assert rc == -1 and lib.hsr_last_error() == b"out_mask is NULL"
    rc = lib.hsr_backward(10, 0, 1, 100, d, 32, 16, d, d, null, d, 1.0, d, null, d, d, d, 1.0, 1.0, null, d, d, d,
                          d, d, d, d, d, d, d, d, d, d, null, null, d, d, null, 0, 0, null)       # shs given, dL_dsh NULL
    assert rc == -1 and lib.hsr_last_error() == b"shs given without dL_dsh / campos"


def test_no_cpu_fallback_and_reference_error_messages():
    """CPU tensors must fail loudly (there is no fallback path); the either/or argument checks keep the
    reference's messages (diff_gaussian_rasterization/__init__.py:195-199)"""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, GaussianRasterizer_semantic
    import scenes
    cam, sc, _ = scenes.build(32, 32, 10, 4)
    rs = GaussianRasterizationSettings(**cam)
    m2 = torch.zeros(10, 3)
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        GaussianRasterizer(rs)(means3D=sc["means3D"], means2D=m2, opacities=sc["opacities"], scales=sc["scales"],
                               rotations=sc["rotations"])
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        GaussianRasterizer_semantic(rs)(means3D=sc["means3D"], means2D=m2, opacities=sc["opacities"],
                                        colors_precomp=sc["colors_precomp"], scales=sc["scales"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        GaussianRasterizer_semantic(rs)(means3D=sc["means3D"], means2D=m2, opacities=sc["opacities"],
                                        colors_precomp=sc["colors_precomp"], scales=sc["scales"], rotations=sc["rotations"],
                                        semantics_precomp=sc["semantics_precomp"])
    with pytest.raises(RuntimeError, match=r"means3D must have dimensions \(num_points, 3\)"):
        GaussianRasterizer(rs)(means3D=torch.zeros(10, 4), means2D=m2, opacities=sc["opacities"],
                               colors_precomp=sc["colors_precomp"], scales=sc["scales"], rotations=sc["rotations"])
    assert GaussianRasterizationSettings._fields == ("image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier",
                                                     "viewmatrix", "projmatrix", "sh_degree", "campos", "prefiltered", "debug")


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
    import importlib
    import sys
    monkeypatch.setenv("HSR_RAST_LIB", str(tmp_path / "nope.so"))
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k.startswith("diff_gaussian_rasterization")}
    try:
        with pytest.raises(ImportError, match="no CPU fallback"):
            importlib.import_module("diff_gaussian_rasterization")
    finally:
        for k in [k for k in sys.modules if k.startswith("diff_gaussian_rasterization")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_camera_matches_reference_convention():
    """setup_camera restatement (utils/recon_helpers.py:4-28): viewmatrix = w2c^T, projmatrix = viewmatrix @ P^T"""
    import numpy as np
    from hsr_utils.camera import replica_intrinsics, setup_camera_tensors
    import scenes
    w2c = scenes.tilted_w2c()
    cam = setup_camera_tensors(1200, 680, replica_intrinsics(), w2c)
    assert np.allclose(cam["viewmatrix"][0].numpy(), w2c.T, atol=1e-7)
    assert abs(cam["tanfovx"] - 1.0) < 1e-12 and abs(cam["tanfovy"] - 680 / 1200.0) < 1e-12
    p = np.array([0.3, -0.2, 2.0, 1.0], np.float32)
    hom = p @ cam["projmatrix"][0].numpy()
    cam_pt = w2c @ p
    assert abs(hom[3] - cam_pt[2]) < 1e-5  # w = view-space depth for this projection
    assert np.allclose(cam["campos"].numpy(), np.linalg.inv(w2c)[:3, 3], atol=1e-6)
