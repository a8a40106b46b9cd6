"""GPU suite for the pictures of a run's mesh (hsr_utils.mesh_view.render_mesh_run, SlamSession.render_mesh, tools/render_mesh.py) on
the short session of tests/test_gpu_mesh_eval.py: the views are the run's own poses and an orbit, the files are the tensors, and the
tool in a fresh process writes what the module writes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import test_gpu_slam_session as TS
from test_gpu_mesh_eval import EVERY, VOXEL, sequence, session  # noqa: F401  (the fixtures: six rendered frames and the short session)

pytestmark = pytest.mark.gpu

SIZE = (64, 48)      # W x H


def picture(path):
    return np.asarray(Image.open(path))


def test_session_renders_its_mesh_from_its_poses_and_an_orbit(session, tmp_path):
    from hsr_utils import mesh, mesh_view, replay
    out = str(tmp_path / "views")
    paths = session.render_mesh(out, voxel_size=VOXEL, mesh_every=EVERY, every=2, orbit=2, pictures=("shaded", "colour", "normals"), size=SIZE)
    T = len(session.gt_w2c_all_frames)
    n_views = len(range(0, T, 2)) + 2
    names = ["%s_%04d.png" % (p, i) for i in range(n_views) for p in ("shaded", "colour", "normals")]
    assert [os.path.basename(p) for p in paths] == names and sorted(os.listdir(out)) == sorted(names + ["mesh.ply"])
    parts = mesh.load_mesh_ply(os.path.join(out, "mesh.ply"))
    assert parts[2] is not None and len(parts[1]) > 100
    # the first view is the run's first estimated pose after first_frame_w2c, at the session's camera scaled to SIZE: the renderer's own bytes
    first = np.asarray(session.first_frame_w2c.cpu().numpy(), np.float32) @ replay.run_w2cs(session.params).cpu().numpy()[0]
    k = np.array(session.intrinsics.cpu().numpy()[:3, :3], np.float64)
    k[0] *= SIZE[0] / session.cam.image_width
    k[1] *= SIZE[1] / session.cam.image_height
    device_parts = [torch.as_tensor(np.ascontiguousarray(p), device="cuda") for p in parts[:3]]
    want = mesh_view.MeshRenderer(device_parts[0], device_parts[1], SIZE[1], SIZE[0], rgb=device_parts[2]).render(first, k, ("shaded", "colour", "normals"))
    for name in ("shaded", "colour", "normals"):
        got = picture(os.path.join(out, "%s_0000.png" % name))
        assert got.shape == (SIZE[1], SIZE[0], 3) and np.array_equal(got, want[name].cpu().numpy()), name
    assert (want["face"] >= 0).float().mean() > 0.3      # the mesh is in view from the pose it was fused from
    orbit = picture(os.path.join(out, "shaded_%04d.png" % (n_views - 1)))
    assert 0 < (orbit != 255).any(-1).mean() < 1      # the orbit sees the mesh against the background
    with pytest.raises(ValueError, match="needs mesh= or voxel_size="):
        session.render_mesh(out)
    again = session.render_mesh(str(tmp_path / "again"), mesh=os.path.join(out, "mesh.ply"), every=2, orbit=2, pictures=("shaded",), size=SIZE)
    assert len(again) == n_views and np.array_equal(picture(again[0]), picture(paths[0])) and np.array_equal(picture(again[-1]), orbit)


def test_the_tool_writes_the_pictures_in_a_fresh_process(session, sequence, tmp_path):  # noqa: F811
    from hsr_utils import map_io, mesh, mesh_view
    cam, intrinsics, frames = sequence
    out = map_io.finalize_params(session.params, session.variables, intrinsics, torch.eye(4), TS.W, TS.H, [f["gt_w2c"] for f in frames],
                                 session.keyframe_time_indices)
    saved = map_io.save_params(out, str(tmp_path / "run"))
    own = session.export_mesh(str(tmp_path / "own.ply"), voxel_size=VOXEL, every=EVERY)
    has_labels = mesh.load_mesh_ply(own[0])[3] is not None
    kinds = ["shaded", "colour", "normals", "scalar"] + (["labels"] if has_labels else [])
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "render_mesh.py")
    done = subprocess.run([sys.executable, tool, own[0], str(tmp_path / "tool"), "--params", saved, "--every", "3", "--orbit", "2", "--pictures",
                           ",".join(kinds), "--gt", own[0], "--size", "%dx%d" % SIZE], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    n_views = len(range(0, len(frames), 3)) + 2
    names = ["%s_%04d.png" % (p, i) for i in range(n_views) for p in kinds + ["gt_shaded"]]
    assert sorted(os.listdir(tmp_path / "tool")) == sorted(names) and "wrote %d pictures" % len(names) in done.stdout
    params = map_io.load_params(saved, device="cuda")
    parts = mesh.load_mesh_ply(own[0])
    paths = mesh_view.render_mesh_run(params, parts, str(tmp_path / "module"), every=3, orbit=2, pictures=tuple(kinds), gt=parts[:2], size=SIZE)
    assert [os.path.basename(p) for p in paths] == names
    for name in names:
        assert np.array_equal(picture(tmp_path / "tool" / name), picture(tmp_path / "module" / name)), name
    for i in range(n_views):      # the ground truth here is the mesh itself: the same shaded picture, and no error anywhere on the heat map
        assert np.array_equal(picture(tmp_path / "tool" / ("gt_shaded_%04d.png" % i)), picture(tmp_path / "tool" / ("shaded_%04d.png" % i)))
    # without --params the views are an orbit at a pinhole of its own: the tool's other branch, in this process
    sys.path.insert(0, os.path.dirname(tool))
    try:
        import render_mesh
        argv, sys.argv = sys.argv, [tool, own[0], str(tmp_path / "orbit"), "--orbit", "3", "--flat", "--size", "%dx%d" % SIZE]
        try:
            render_mesh.main()
        finally:
            sys.argv = argv
    finally:
        sys.path.remove(os.path.dirname(tool))
    assert sorted(os.listdir(tmp_path / "orbit")) == ["shaded_%04d.png" % i for i in range(3)]
    assert all(0 < (picture(tmp_path / "orbit" / ("shaded_%04d.png" % i)) != 255).any(-1).mean() < 1 for i in range(3))
