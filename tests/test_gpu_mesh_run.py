"""GPU suite for the mesh of a run end to end (hsr_utils.mesh.mesh_run, SlamSession.export_mesh, tools/mesh_run.py) on the six-frame
sequence of tests/test_gpu_slam_session.py: a short session's map rendered from its estimated poses, fused and extracted.  The kernels
themselves are pinned in tests/test_gpu_tsdf.py; here the file, the loop and its defaults are."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_gpu_slam_session as TS
from test_gpu_slam_session import sequence  # noqa: F401  (the fixture: six rendered frames of a hidden map)

pytestmark = pytest.mark.gpu

VOXEL, EVERY = 0.08, 2


@pytest.fixture(scope="module")
def session(sequence):  # noqa: F811
    """a short session over all six frames (2 tracking and 2 mapping iterations a frame) and the mesh it exports"""
    from hsr_utils import SlamSession
    cam, intrinsics, frames = sequence
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    config = TS._config(2)
    config["mapping"]["num_iters"] = 2
    s = SlamSession(config, intrinsics, torch.eye(4, device="cuda"), cam)
    for frame in frames:
        s.step(frame)
    return s


@pytest.fixture(scope="module")
def exported(session, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("mesh") / "session.ply")
    return session.export_mesh(path, voxel_size=VOXEL, every=EVERY)


def test_export_mesh_writes_a_mesh_that_loads(session, exported):
    from hsr_utils import mesh
    path, nv, nf = exported
    vertices, faces, rgb, labels = mesh.load_mesh_ply(path)
    assert (nv, nf) == (len(vertices), len(faces)) and nf > 0 and nv > 0
    assert faces.min() >= 0 and faces.max() < nv and len(np.unique(faces)) == nv      # every index names a vertex, every vertex is used
    assert rgb is not None and rgb.shape == (nv, 3) and labels is not None and labels.shape == (nv,)      # a semantic session: both
    assert np.isfinite(vertices).all()
    lo = session.params["means3D"].detach().min(dim=0).values.cpu().numpy() - 4 * VOXEL - 1e-4
    hi = session.params["means3D"].detach().max(dim=0).values.cpu().numpy() + 4 * VOXEL + VOXEL
    assert (vertices >= lo).all() and (vertices <= hi).all()      # inside the padded box of the map
    assert ((labels >= 0) & (labels < TS.K)).all()      # "flat": the argmax over the K planes
    print("session mesh: %d vertices, %d faces" % (nv, nf))


def test_export_mesh_equals_the_volume_driven_by_hand(session, exported, tmp_path):
    """session.render(t) of every second frame into a TsdfVolume over mesh_bounds, then extract and save: the same bytes"""
    from hsr_utils import evaluate, mesh, slam
    s = session
    origin, dims = mesh.mesh_bounds(s.params, 4 * VOXEL, VOXEL)
    vol = mesh.TsdfVolume(origin, dims, VOXEL, labels=True)
    for t in range(0, TS.FRAMES, EVERY):
        im, depth, opac, sem = s.render(t)
        labels = evaluate.semantic_labels(sem, "flat").to(torch.int64)
        vol.integrate(depth, slam.frame_w2c(s.params, t), s.intrinsics, color=im, labels=labels, opacity=opac, sil_thres=0.5)
    assert float(vol.weight.max()) == len(range(0, TS.FRAMES, EVERY)) and (vol.weight == 0).any()
    path = mesh.save_mesh_ply(str(tmp_path / "hand.ply"), *vol.extract())
    assert open(path, "rb").read() == open(exported[0], "rb").read()


def test_two_exports_and_the_saved_run_give_the_same_file(session, sequence, exported, tmp_path):  # noqa: F811
    from hsr_utils import map_io, mesh
    s = session
    cam, intrinsics, frames = sequence
    want = open(exported[0], "rb").read()
    again = s.export_mesh(str(tmp_path / "again.ply"), voxel_size=VOXEL, every=EVERY)
    assert again[1:] == exported[1:] and open(again[0], "rb").read() == want
    out = map_io.finalize_params(s.params, s.variables, intrinsics, torch.eye(4), TS.W, TS.H, [f["gt_w2c"] for f in frames], s.keyframe_time_indices)
    saved = map_io.save_params(out, str(tmp_path / "run"))
    params = map_io.load_params(saved, device="cuda")
    # with the camera the session rendered with (its projection was built from float64 intrinsics; the file keeps float32 ones)
    got = mesh.mesh_run(params, str(tmp_path / "saved.ply"), voxel_size=VOXEL, every=EVERY, semantic=True, cam=cam)
    assert got[1:] == exported[1:] and open(got[0], "rb").read() == want
    # other settings give another mesh: no labels without semantic=True, more views with every=1
    plain = mesh.mesh_run(params, str(tmp_path / "plain.ply"), voxel_size=VOXEL, every=1, cam=cam)
    vertices, faces, rgb, labels = mesh.load_mesh_ply(plain[0])
    assert labels is None and rgb is not None and len(faces) > 0 and faces.max() < len(vertices)
    with pytest.raises(ValueError, match="more than max_voxels = 1000; a voxel size of"):
        mesh.mesh_run(params, str(tmp_path / "big.ply"), voxel_size=VOXEL, max_voxels=1000)
    assert not os.path.exists(str(tmp_path / "big.ply"))


def test_the_tool_in_a_fresh_process(session, sequence, tmp_path):  # noqa: F811
    from hsr_utils import map_io, mesh
    s = session
    _cam, intrinsics, frames = sequence
    out = map_io.finalize_params(s.params, s.variables, intrinsics, torch.eye(4), TS.W, TS.H, [f["gt_w2c"] for f in frames], s.keyframe_time_indices)
    saved = map_io.save_params(out, str(tmp_path / "run"))
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "mesh_run.py")
    target = str(tmp_path / "tool.ply")
    done = subprocess.run([sys.executable, tool, saved, target, "--voxel-size", str(VOXEL), "--every", str(EVERY), "--semantic"],
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    vertices, faces, rgb, labels = mesh.load_mesh_ply(target)
    assert "wrote %d vertices and %d faces to %s" % (len(vertices), len(faces), target) in done.stdout
    assert len(faces) > 0 and faces.max() < len(vertices) and rgb is not None and labels is not None
