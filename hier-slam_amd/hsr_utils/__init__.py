"""Host-side helpers around the rasterizer path: camera construction and synthetic scenes.

These mirror caller-side conventions of the reference (utils/recon_helpers.py:4-28,
scripts/hierslam.py:361-389) so that tests and bench.py feed the rasterizer the same
shapes and layouts scripts/hierslam.py does.  Nothing here computes on the hot path.
"""
from .camera import setup_camera_tensors, setup_camera, scale_intrinsics  # noqa: F401
from .synthetic import make_scene, make_upstream_grads  # noqa: F401

_KEYFRAMES = ("keyframe_selection_overlap", "overlap_counts", "KeyframePoses", "mapping_window")
_SLAM = ("initialize_first_timestep", "initialize_camera_pose", "update_poses", "matrix_to_quaternion", "is_keyframe", "SlamSession",
         "resample_frame", "render_view")
_FRAMES = ("tree_label_table", "ingest_frame", "ingest_frame_planes", "composed_label_table", "ingest_frame_undistort")
_SEQUENCE = ("ReplicaSequence", "tree_annotation", "ScanNetSequence", "scannet_class_mapping", "scannet_tree_annotation",
             "ReplicaV2Sequence", "TUMSequence")
_EXPORT = ("export_frame", "jet_colormap", "label_colormap", "tuple_colour_table", "write_png")
_MAP_EXPORT = ("export_map", "gaussian_tree_labels", "level_prefix_colour_table", "leaf_head_labels", "save_map_ply",
               "save_map_ply_semantic")
_REPLAY = ("run_w2cs", "ReplayPlan", "replay_rendervars", "replay_view", "view_cloud", "save_cloud_ply", "follow_camera", "camera_centres",
           "trajectory_lines", "replay_run")
_CHECKPOINT = ("PackedKeyframe", "pack_keyframe", "unpack_keyframe", "save_checkpoint", "load_checkpoint")
_MESH = ("TsdfVolume", "mesh_bounds", "save_mesh_ply", "load_mesh_ply", "mesh_run")
_MESH_EVAL = ("face_areas", "sample_mesh", "NearestGrid", "seen_vertices", "cull_mesh", "distance_metrics", "label_metrics", "mesh_metrics",
              "evaluate_mesh_run")
_MESH_DEPTH = ("MeshDepthRenderer", "render_mesh_depth", "virtual_views", "mesh_depth_l1")
_MESH_CLEAN = ("mesh_components", "component_keep", "clean_mesh")
_MESH_ALIGN = ("rigid_from_sums", "icp_step", "icp", "trajectory_alignment", "transform_points", "align_mesh")
_MESH_VIEW = ("vertex_normals", "MeshRenderer", "vertex_errors", "orbit_views", "render_mesh_views", "render_mesh_run")


def __getattr__(name):
    # the keyframe selection binds libhsr_rast.so: resolved on first use, so that importing the host-side helpers above stays library-free
    if name in _KEYFRAMES:
        from . import keyframes
        return getattr(keyframes, name)
    if name in _SLAM:      # the loop driver binds the library too
        from . import slam
        return getattr(slam, name)
    if name in _FRAMES:    # so does the ingest of raw sensor frames
        from . import frames
        return getattr(frames, name)
    if name in _SEQUENCE:  # host only (PIL): resolved on first use like the rest
        from . import sequence
        return getattr(sequence, name)
    if name in _EXPORT:    # the pictures of an evaluated frame: binds the library as well
        from . import export
        return getattr(export, name)
    if name in _MAP_EXPORT:      # and the map as PLY records
        from . import map_export
        return getattr(map_export, name)
    if name in _REPLAY:          # and the replay of a finished run
        from . import replay
        return getattr(replay, name)
    if name in _CHECKPOINT:      # and the packed keyframe store with a session's checkpoint and resume
        from . import checkpoint
        return getattr(checkpoint, name)
    if name in _MESH:            # and the mesh of a finished run
        from . import mesh
        return getattr(mesh, name)
    if name in _MESH_EVAL:       # and that mesh scored against a ground-truth mesh
        from . import mesh_eval
        return getattr(mesh_eval, name)
    if name in _MESH_DEPTH:      # and both meshes as depth images from views the sensor never took
        from . import mesh_depth
        return getattr(mesh_depth, name)
    if name in _MESH_CLEAN:      # and the run's mesh without its small disconnected pieces
        from . import mesh_clean
        return getattr(mesh_clean, name)
    if name in _MESH_ALIGN:      # and that mesh registered to the ground truth before it is scored
        from . import mesh_align
        return getattr(mesh_align, name)
    if name in _MESH_VIEW:       # and pictures of either mesh without a window
        from . import mesh_view
        return getattr(mesh_view, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
