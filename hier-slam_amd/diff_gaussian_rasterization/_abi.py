"""The C ABI of libhsr_rast.so as ctypes sees it: the library handle, the structures of the headers, the signature of every exported
function, and the one way a stream-taking entry point is called.

Everything under include/hsr_*.h, include/ext/, include/eval/, include/recon/, include/sensor/, include/surface/, include/align/ and include/shade/ is declared HERE and nowhere else; `_C.py` and the hsr_utils modules
import from this module.  One rule: HEADERS maps each header, by its path under include/, to the signatures of that header's functions, in the
header's order.  The entries are written out by hand (nothing parses a header at import: the package does not depend on where
include/ sits at run time); tests/test_abi.py parses every header on disk and fails on a header without a key, a key without a
header, a name out of the header's order or bound twice, and any entry whose type class differs from its prototype's.  There is NO
fallback path: a missing library is an ImportError.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HSR_RAST_LIB", os.path.join(os.path.dirname(_HERE), "libhsr_rast.so"))

HSR_ERR_BUFFER_TOO_SMALL = -2
HSR_PENDING = -100
HSR_SCRATCH_AS_PLANNED = C.c_size_t(-1).value

vp, ci, cu, cf, cd, sz, cs = C.c_void_p, C.c_int, C.c_uint, C.c_float, C.c_double, C.c_size_t, C.c_char_p
ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)      # HOST arrays (level_sizes, level_weight)


# ---- structures, named and laid out as the header typedefs -------------------------------------------------------------------------
class hsr_buffer(C.Structure):
    _fields_ = [("ptr", vp), ("capacity", sz), ("grow", vp), ("user", vp)]


GROW_FN = C.CFUNCTYPE(vp, sz, vp)      # hsr_grow_fn


class hsr_ticket(C.Structure):
    """a forward call that returned before num_rendered was known"""
    _fields_ = [("seq", C.c_uint32), ("device", C.c_int32), ("slot", vp), ("binning_base", vp), ("binning_capacity", sz),
                ("prefiltered", C.c_int32), ("rendered", C.c_int32)]


class hsr_state_layout(C.Structure):
    _fields_ = [(n, sz) for n in (
        "geom_depths", "geom_means2D", "geom_conic_opacity", "geom_cov3D", "geom_rgb", "geom_clamped",
        "geom_tiles_touched", "geom_point_offsets", "geom_radii",
        "bin_keys_unsorted", "bin_keys", "bin_vals_unsorted", "bin_vals",
        "img_ranges", "img_final_T", "img_n_contrib", "img_median_pos")]


class hsr_backward_plan(C.Structure):
    """what one backward call will do (hsr_plan_backward); kernel: 0 Q-panel, 1 Q-geo, 2 subw, 3 all-VALU"""
    _fields_ = [("accumulation", C.c_int), ("kernel", C.c_int), ("row_layout", C.c_int), ("row_stride", C.c_int),
                ("geometry_only", C.c_int), ("semantic_alpha", C.c_int), ("scratch_bytes", C.c_size_t)]


class hsr_row_table(C.Structure):
    _fields_ = [("src", vp), ("append", vp), ("dst", vp), ("cols", ci)]


class hsr_adam_tensor(C.Structure):
    _fields_ = [("param", vp), ("grad", vp), ("exp_avg", vp), ("exp_avg_sq", vp), ("numel", C.c_int64),
                ("step_size", cf), ("bc2_sqrt", cf), ("eps", cf), ("one_minus_beta1", cf), ("beta2", cf), ("one_minus_beta2", cf)]


class hsr_ingest_level(C.Structure):
    """one output level of hsr_frame_ingest (include/ext/hsr_frame_ingest.h)"""
    _fields_ = [("H", ci), ("W", ci), ("color", vp), ("depth", vp)]


class hsr_export_job(C.Structure):
    """one picture of hsr_frame_export (include/ext/hsr_frame_export.h)"""
    _fields_ = [("kind", ci), ("src", vp), ("table", vp), ("n", ci), ("K", ci), ("L", ci), ("sizes", ci * 16), ("lo", cf), ("hi", cf),
                ("out", vp)]


class hsr_map_export_job(C.Structure):
    """the one job of hsr_map_export (include/ext/hsr_map_export.h)"""
    _fields_ = [("P", ci), ("S", ci), ("record", ci), ("colour", ci), ("means3D", vp), ("rgb_colors", vp), ("unnorm_rotations", vp),
                ("logit_opacities", vp), ("log_scales", vp), ("normals", vp), ("colours", vp), ("labels", vp), ("semantic", vp),
                ("table", vp), ("n", ci), ("K", ci), ("L", ci), ("sizes", ci * 16), ("out", vp), ("out_labels", vp)]


class hsr_shade_job(C.Structure):
    """one picture of hsr_mesh_shade (include/shade/hsr_mesh_shade.h)"""
    _fields_ = [("kind", ci), ("lit", ci), ("normals", vp), ("attr", vp), ("table", vp), ("n", ci), ("lo", cf), ("hi", cf), ("ambient", cf),
                ("albedo", cf * 3), ("background", C.c_uint8 * 4), ("out", vp)]


bp, tk = C.POINTER(hsr_buffer), C.POINTER(hsr_ticket)

# ---- signatures: header (its path under include/) -> (name, restype, argtypes) of each of its functions, in the header's order, -----
# ---- broken into lines where the prototype breaks ----------------------------------------------------------------------------------
HEADERS = {
    "hsr_rasterizer.h": (
        ("hsr_required_geometry_bytes", sz, [ci]),
        ("hsr_required_image_bytes", sz, [ci, ci]),
        ("hsr_required_binning_bytes", sz, [ci]),
        ("hsr_backward_scratch_bytes", sz, [ci, ci, ci]),
        ("hsr_set_backward_mode", ci, [ci]),
        ("hsr_get_backward_mode", ci, []),
        ("hsr_plan_backward", ci, [ci, ci, ci, sz, C.POINTER(hsr_backward_plan)]),
        ("hsr_set_semantic_alpha_mode", ci, [ci]),
        ("hsr_get_semantic_alpha_mode", ci, []),
        ("hsr_last_error", cs, []),
        ("hsr_version", cs, []),
        ("hsr_mark_visible", ci, [ci, vp, vp, vp,
                                  vp, vp]),
        ("hsr_forward", ci, [bp, bp, bp,
                             ci, ci, ci, vp, ci, ci,
                             vp, vp, vp, vp,
                             vp, cf, vp, vp,
                             vp, vp, vp,
                             cf, cf, ci,
                             vp, vp, vp, vp, vp,
                             vp, ci, vp]),
        ("hsr_forward_semantic", ci, [bp, bp, bp,
                                      ci, ci, ci, ci, vp, ci, ci,
                                      vp, vp, vp,
                                      vp, vp,
                                      vp, cf, vp, vp,
                                      vp, vp, vp,
                                      cf, cf, ci,
                                      vp, vp, vp, vp,
                                      vp, vp, ci, vp]),
        ("hsr_forward_arm_async", ci, [tk]),
        ("hsr_forward_end", ci, [tk, ci, vp]),
        ("hsr_backward", ci, [ci, ci, ci, ci, vp, ci, ci,
                              vp, vp, vp,
                              vp, cf, vp, vp,
                              vp, vp, vp,
                              cf, cf, vp,
                              vp, vp, vp,
                              vp, vp, vp,
                              vp,
                              vp, vp, vp, vp, vp,
                              vp, vp, vp, vp, vp,
                              vp, sz, ci, vp]),
        ("hsr_backward_semantic", ci, [ci, ci, ci, ci, ci, vp, ci, ci,
                                       vp, vp, vp,
                                       vp,
                                       vp, cf, vp, vp,
                                       vp, vp, vp,
                                       cf, cf, vp,
                                       vp, vp, vp,
                                       vp, vp, vp,
                                       vp, vp,
                                       vp, vp, vp, vp,
                                       vp, vp,
                                       vp, vp, vp, vp, vp,
                                       vp, sz, ci, vp]),
        ("hsr_get_state_layout", ci, [ci, ci, ci, ci, C.POINTER(hsr_state_layout)]),
        ("hsr_profile_enable", ci, [ci]),
        ("hsr_profile_select", ci, [cu]),
        ("hsr_profile_read", ci, [vp, ci]),
        ("hsr_stage_name", cs, [ci]),
        ("hsr_profile_host_wait_ms", cd, [ci]),
    ),
    "hsr_frame_prep.h": (
        ("hsr_frame_prep_scratch_bytes", sz, [ci]),
        ("hsr_frame_prep_forward", ci, [ci, ci, ci, ci, vp, vp,
                                        vp, vp, vp,
                                        vp, ci, ci, vp, vp,
                                        vp, vp, vp, vp,
                                        vp, vp]),
        ("hsr_frame_prep_backward", ci, [ci, ci, ci, ci, vp, vp,
                                         vp, vp, vp,
                                         vp, ci, ci, vp,
                                         vp, vp, vp,
                                         vp, vp, vp,
                                         vp, vp, vp, vp,
                                         vp, vp, vp, sz, vp]),
        ("hsr_frame_prep_backward_params", ci, [ci, ci, ci, ci, vp, vp,
                                                vp, vp, vp,
                                                vp, ci, ci, vp,
                                                vp, vp, vp,
                                                vp, vp, vp,
                                                vp, vp, vp, vp,
                                                vp, vp, vp, sz, vp]),
    ),
    "hsr_losses.h": (
        ("hsr_loss_scratch_bytes", sz, [ci, ci, ci]),
        ("hsr_loss_l1", ci, [ci, ci, ci, vp, vp, vp, ci, vp,
                             vp, vp, sz, vp]),
        ("hsr_loss_tracking_scratch_bytes", sz, [ci, ci]),
        ("hsr_loss_tracking_value", ci, [ci, ci, ci, vp, vp, vp, vp,
                                         vp, cf, ci, ci, cf, cf, vp,
                                         vp, sz, vp]),
        ("hsr_loss_tracking_grad", ci, [ci, ci, ci, vp, vp, vp, vp,
                                        vp, cf, ci, cf, cf, vp,
                                        vp, vp, vp, vp]),
        ("hsr_loss_ssim", ci, [ci, ci, ci, vp, vp, vp, vp, vp,
                               sz, vp]),
        ("hsr_loss_l1_grad", ci, [ci, ci, ci, vp, vp, vp, ci, vp,
                                  vp, vp]),
        ("hsr_loss_ssim_value", ci, [ci, ci, ci, vp, vp, vp, vp, vp,
                                     sz, vp]),
        ("hsr_loss_ssim_grad", ci, [ci, ci, ci, vp, vp, vp, vp, vp,
                                    vp]),
        ("hsr_loss_tree_ce", ci, [ci, ci, ci, ci, ip, fp, vp,
                                  vp, ci, vp, vp, vp,
                                  sz, vp]),
        ("hsr_loss_tree_ce_scratch_bytes", sz, [ci, ci]),
        ("hsr_loss_tree_ce_value", ci, [ci, ci, ci, ci, ip, vp, vp,
                                        ci, vp, vp, vp, sz,
                                        vp]),
        ("hsr_loss_tree_ce_grad", ci, [ci, ci, ci, ci, ip, fp, vp,
                                       vp, ci, vp, vp, vp,
                                       vp, cf, vp, vp]),
        ("hsr_loss_leaf_mlp_ce", ci, [ci, ci, ci, ci, vp, vp, vp, vp,
                                      ci, vp, vp, vp, vp, vp,
                                      sz, vp]),
    ),
    "hsr_densify.h": (
        ("hsr_densify_scratch_bytes", sz, [ci, ci]),
        ("hsr_densify_frame", ci, [ci, ci, vp, vp, vp, vp,
                                   cf, cf, cf, cf, vp, cf, cf, ci,
                                   vp, vp, vp, vp, vp,
                                   vp, vp, vp, sz, vp]),
        ("hsr_compact_scratch_bytes", sz, [ci]),
        ("hsr_prune_mask", ci, [ci, ci, vp, vp, cf,
                                cf, vp, vp, vp, sz, vp]),
        ("hsr_compact_append_rows", ci, [ci, vp, ci, ci, C.POINTER(hsr_row_table), ci,
                                         vp, vp, sz, vp]),
    ),
    "hsr_eval.h": (
        ("hsr_eval_metrics_scratch_bytes", sz, [ci, ci]),
        ("hsr_eval_frame_metrics", ci, [ci, ci, vp, vp, vp, vp,
                                        vp, cf, vp, vp, sz, vp]),
        ("hsr_eval_labels_flat", ci, [ci, ci, ci, vp, vp, vp]),
        ("hsr_eval_labels_tree", ci, [ci, ci, ci, ci, ip, vp, vp,
                                      vp, vp, vp]),
        ("hsr_eval_leaf_scratch_bytes", sz, [ci]),
        ("hsr_eval_labels_leaf", ci, [ci, ci, ci, ci, vp, vp, vp, vp,
                                      vp, sz, vp]),
        ("hsr_eval_iou_scratch_bytes", sz, [ci, ci]),
        ("hsr_eval_iou_counts", ci, [ci, ci, vp, vp, ci, vp, vp,
                                     ci, vp, vp, sz, vp]),
        ("hsr_eval_frame_miou", ci, [ci, vp, vp, vp]),
    ),
    "hsr_optim.h": (
        ("hsr_adam_table_entry_bytes", sz, []),
        ("hsr_adam_step", ci, [ci, C.POINTER(hsr_adam_tensor), vp]),
        ("hsr_track_keep_best", ci, [ci, ci, vp, vp, vp, vp,
                                     vp, vp, vp]),
    ),
    "hsr_keyframes.h": (
        ("hsr_kf_valid_rows", ci, [ci, ci, vp, vp, vp]),
        ("hsr_kf_sample_scratch_bytes", sz, [ci]),
        ("hsr_kf_sample_points", ci, [ci, ci, vp, vp, ci, vp, cf, cf,
                                      cf, cf, vp, vp, vp, vp,
                                      vp, vp, sz, vp]),
        ("hsr_kf_round_keys", ci, [ci, vp, vp, vp]),
        ("hsr_kf_overlap_counts", ci, [ci, vp, vp, ci, vp, vp, ci,
                                       ci, ci, vp, vp]),
    ),
    # ---- extensions: the headers under include/ext/ ------------------------------------------------------------------------------------
    "ext/hsr_msssim.h": (
        ("hsr_eval_msssim_scratch_bytes", sz, [ci, ci]),
        ("hsr_eval_msssim", ci, [ci, ci, vp, vp, vp, vp,
                                 cf, vp, vp, sz, vp]),
    ),
    "ext/hsr_map_init.h": (
        ("hsr_map_init_scratch_bytes", sz, [ci, ci]),
        ("hsr_map_init_frame", ci, [ci, ci, vp, vp, cf, cf, cf, cf, vp,
                                    cf, ci, ci, vp, vp, vp,
                                    vp, vp, vp, vp,
                                    vp, sz, vp]),
    ),
    "ext/hsr_frame_resample.h": (
        ("hsr_frame_resample", ci, [ci, ci, vp, vp, ci, ci, vp, vp,
                                    ci, ci, vp, vp, vp]),
    ),
    "ext/hsr_loss_outlier.h": (
        ("hsr_loss_outlier_scratch_bytes", sz, [ci, ci]),
        ("hsr_loss_outlier_median", ci, [ci, ci, vp, vp, vp, vp, sz,
                                         vp]),
        ("hsr_loss_outlier_value", ci, [ci, ci, ci, vp, vp, vp, vp,
                                        vp, cf, ci, ci, cf, cf, vp,
                                        vp, vp, sz, vp]),
        ("hsr_loss_outlier_grad", ci, [ci, ci, ci, vp, vp, vp, vp,
                                       vp, cf, ci, cf, cf, vp,
                                       vp, vp, vp, vp, vp]),
    ),
    "ext/hsr_frame_ingest.h": (
        ("hsr_frame_ingest", ci, [ci, ci, vp, vp, ci, cd,
                                  vp, ci, vp, ci,
                                  ci, C.POINTER(hsr_ingest_level), vp, vp]),
    ),
    "ext/hsr_frame_export.h": (
        ("hsr_frame_export", ci, [ci, ci, ci, C.POINTER(hsr_export_job), vp]),
    ),
    # the ingest with a source size per image
    "ext/hsr_frame_ingest_planes.h": (
        ("hsr_frame_ingest_planes", ci, [ci, ci, vp,
                                         ci, ci, vp, ci, cd,
                                         ci, ci, vp,
                                         ci, vp, ci, ci,
                                         ci, C.POINTER(hsr_ingest_level), vp, vp]),
    ),
    # the map as PLY records
    "ext/hsr_map_export.h": (
        ("hsr_map_export", ci, [C.POINTER(hsr_map_export_job), vp]),
    ),
    # rasterizer inputs from a given world-to-camera matrix and a view's hole counts
    "ext/hsr_view.h": (
        ("hsr_view_prep", ci, [ci, ci, ci, ci,
                               vp, vp,
                               vp, vp,
                               vp,
                               vp, vp, vp,
                               vp, vp, vp]),
        ("hsr_view_holes_scratch_bytes", sz, [ci, ci]),
        ("hsr_view_holes", ci, [ci, ci, vp, vp, cf,
                                vp, vp, sz, vp]),
    ),
    # the map as it stood at step t and a view's point cloud
    "ext/hsr_replay.h": (
        ("hsr_replay_plan_scratch_bytes", sz, [ci, ci]),
        ("hsr_replay_plan", ci, [ci, ci, vp, vp,
                                 vp, sz, vp]),
        ("hsr_replay_select_scratch_bytes", sz, [ci]),
        ("hsr_replay_select", ci, [ci, ci, ci, ci, ci, ci, ci,
                                   vp, vp, vp, vp,
                                   vp, vp, vp, vp,
                                   vp, vp, vp, vp, vp,
                                   vp, vp, vp, vp,
                                   vp, sz, vp]),
        ("hsr_replay_cloud", ci, [ci, ci, vp, vp, cf, cf, cf, cf,
                                  vp, vp, vp, vp]),
    ),
    # a keyframe's planes as 8-/16-bit codes and back
    "ext/hsr_keyframe_pack.h": (
        ("hsr_keyframe_pack_scratch_bytes", sz, [ci, ci, ci]),
        ("hsr_keyframe_pack", ci, [ci, ci, vp, vp, ci, vp, cd,
                                   vp, vp, vp, vp,
                                   vp, sz, vp]),
        ("hsr_keyframe_unpack", ci, [ci, ci, vp, vp, ci, vp,
                                     cd, vp, vp, vp, vp]),
    ),
    # depth fused into a signed distance volume and its surface (w2c is a HOST array)
    "ext/hsr_tsdf.h": (
        ("hsr_tsdf_integrate", ci, [ci, ci, ci, cf, cf, cf, cf, cf, cf,
                                    ci, ci, cf, cf, cf, cf, fp,
                                    vp, vp, vp, vp, cf, cf,
                                    vp, vp, vp, vp, vp, vp, vp]),
        ("hsr_tsdf_count", ci, [ci, ci, ci, vp, vp, vp, vp]),
        ("hsr_tsdf_faces", ci, [ci, ci, ci, vp, vp, vp, sz, vp,
                                vp]),
        ("hsr_tsdf_vertices", ci, [ci, ci, ci, cf, cf, cf, cf, sz, vp,
                                   vp, vp, vp, vp,
                                   vp, vp, vp, vp]),
    ),
}

# ---- the headers under include/eval/, a second table of the same shape: HEADERS above is a counted set (tests/test_abi.py), and the
# ---- suite of each header here checks it with the same helpers (tests/test_mesh_eval_cpu.py) ----------------------------------------
EVAL_HEADERS = {
    # a run's mesh against a ground-truth mesh: areas, surface samples, seen vertices, exact nearest neighbours (w2c is a HOST array;
    # the seed is a 64-bit word)
    "eval/hsr_mesh_eval.h": (
        ("hsr_mesh_areas", ci, [ci, ci, vp, vp, vp, vp]),
        ("hsr_mesh_sample", ci, [ci, ci, ci, sz, vp, vp, vp,
                                 vp, vp, vp, vp, vp]),
        ("hsr_mesh_seen", ci, [ci, vp, ci, ci, cf, cf, cf, cf, fp,
                               vp, cf, vp, vp]),
        ("hsr_nn_cells", ci, [ci, ci, ci, cf, cf, cf, cf, ci, vp, vp, vp]),
        ("hsr_nn_pack", ci, [ci, vp, vp, vp, vp]),
        ("hsr_nn_query", ci, [ci, ci, ci, cf, cf, cf, cf, ci, vp, vp,
                              ci, vp, vp, vp, vp]),
    ),
}

# ---- the headers under include/recon/, a third table of the same shape: EVAL_HEADERS above is a counted set too
# ---- (tests/test_mesh_eval_cpu.py); tests/test_mesh_depth_cpu.py checks this one with the same helpers ------------------------------
RECON_HEADERS = {
    # the depth image of a triangle mesh from one view (w2c is a HOST array)
    "recon/hsr_mesh_depth.h": (
        ("hsr_mesh_depth_scratch_bytes", sz, [ci, ci, ci]),
        ("hsr_mesh_depth", ci, [ci, ci, vp, vp, ci, ci, cf, cf, cf, cf,
                                fp, cf, vp, sz, vp, vp, vp]),
    ),
}

# ---- the headers under include/sensor/, a fourth table of the same shape: RECON_HEADERS above is a counted set too
# ---- (tests/test_mesh_depth_cpu.py); tests/test_frame_undistort_cpu.py checks this one with the same helpers -------------------------
SENSOR_HEADERS = {
    # the ingest with the colour image undistorted on the way: the camera of the sensor image and five coefficients, all double
    "sensor/hsr_frame_undistort.h": (
        ("hsr_frame_ingest_undistort", ci, [ci, ci, vp, vp, ci, cd,
                                            vp, ci, vp, ci,
                                            cd, cd, cd, cd,
                                            cd, cd, cd, cd, cd,
                                            ci, C.POINTER(hsr_ingest_level), vp, vp]),
    ),
}

# ---- the headers under include/surface/, a fifth table of the same shape: SENSOR_HEADERS above is a counted set too
# ---- (tests/test_frame_undistort_cpu.py); tests/test_mesh_clean_cpu.py checks this one with the same helpers ---------------------------
SURFACE_HEADERS = {
    # the connected components of a mesh and the faces and vertices of the kept ones (out_counts is three 64-bit words on the device)
    "surface/hsr_mesh_clean.h": (
        ("hsr_mesh_components", ci, [ci, ci, vp, vp, vp, vp]),
        ("hsr_mesh_select_scratch_bytes", sz, [ci, ci]),
        ("hsr_mesh_select", ci, [ci, ci, vp, vp, vp, vp, vp,
                                 vp, vp, sz, vp]),
    ),
}

# ---- the headers under include/align/, a sixth table of the same shape: SURFACE_HEADERS above is a counted set too
# ---- (tests/test_mesh_clean_cpu.py); tests/test_mesh_align_cpu.py checks this one with the same helpers ---------------------------------
ALIGN_HEADERS = {
    # one pass of point-to-point ICP against the grid of hsr_nn_query (transform is a HOST array of 12 floats; out_sums is 17 float64)
    "align/hsr_mesh_align.h": (
        ("hsr_icp_scratch_bytes", sz, [ci]),
        ("hsr_icp_step", ci, [ci, ci, ci, cf, cf, cf, cf, ci, vp, vp,
                              ci, vp, fp, cf, vp, vp,
                              vp, vp, sz, vp]),
    ),
}

# ---- the headers under include/shade/, a seventh table of the same shape: ALIGN_HEADERS above is a counted set too
# ---- (tests/test_mesh_align_cpu.py); tests/test_mesh_view_cpu.py checks this one with the same helpers -----------------------------------
SHADE_HEADERS = {
    # vertex normals and the pictures of a mesh from one view (w2c and jobs are HOST arrays)
    "shade/hsr_mesh_shade.h": (
        ("hsr_mesh_normals_scratch_bytes", sz, [ci]),
        ("hsr_mesh_normals", ci, [ci, ci, vp, vp, vp, sz, vp,
                                  vp]),
        ("hsr_mesh_shade", ci, [ci, ci, vp, vp, ci, ci, cf, cf, cf, cf,
                                fp, vp, ci, C.POINTER(hsr_shade_job), vp]),
    ),
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "diff_gaussian_rasterization: HIP library not found at %s — build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C hier-slam_amd/csrc`. "
            "There is no CPU fallback." % LIB_PATH)
    loaded = C.CDLL(LIB_PATH)
    for table in (list(HEADERS.values()) + list(EVAL_HEADERS.values()) + list(RECON_HEADERS.values()) + list(SENSOR_HEADERS.values())
                  + list(SURFACE_HEADERS.values()) + list(ALIGN_HEADERS.values()) + list(SHADE_HEADERS.values())):
        for name, restype, argtypes in table:
            fn = getattr(loaded, name)
            fn.restype, fn.argtypes = restype, argtypes
    return loaded


lib = _load()


def fail(rc, what):
    raise RuntimeError("%s failed (code %d): %s" % (what, rc, lib.hsr_last_error().decode()))


def call(fn, what, dev, *args):
    """fn(*args, stream) for an entry point that ends in `void* stream`: on device `dev`, on its current stream; raises on a negative
    return code.  Pass `lib.hsr_x` itself, looked up at the call, so that a replaced attribute of `lib` is what runs."""
    with torch.cuda.device(dev):
        rc = fn(*args, torch.cuda.current_stream(dev).cuda_stream)
    if rc < 0:
        fail(rc, what)
