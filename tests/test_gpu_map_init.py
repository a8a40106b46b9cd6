"""GPU suite for the first-frame map (include/ext/hsr_map_init.h, hsr_utils.slam.map_init_frame / initialize_first_timestep) against an
fp32 torch restatement, written here and run on the device, of get_pointcloud(mask = depth > 0, compute_mean_sq_dist = True)
(scripts/hierslam.py:144-194) + initialize_params (:322-359) + scene_radius (:456), in the reference's operation order.

Bit for bit: the count, the row order, colours, rotations, opacities and scene_radius.  means3D and log_scales (= log(sqrt(mean3_sq_dist)),
the only form in which the kernel hands mean3_sq_dist out) are bit-equal too where the kernel's plain IEEE chain and torch's agree; the
means go through torch's matmul, whose accumulation order and contraction are the BLAS library's, so where they are not bit-equal the kernel's
distance from a float64 restatement on the same inputs is held to twice the fp32 restatement's own distance from it.  Every figure is printed.

Shapes: 1x1; 7x5; 64x48 with 30 % zero or negative depth; 37x23 (851 pixels: four 256-pixel blocks, the last one partial); 515x511 (1028
blocks: the single-workgroup scan takes two blocks per thread); all-invalid depth; capacity < M; S = 1 and 3; identity, tilted and general c2w."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RATIO = 3.0      # scene_radius_depth_ratio of the reference's configs

#        name            H    W    S  invalid  tilted
CASES = [("1x1",          1,   1,   1, 0.0,     True),
         ("7x5",          7,   5,   3, 0.0,     False),
         ("64x48_holes",  64,  48,  1, 0.3,     True),
         ("37x23",        37,  23,  3, 0.1,     True),
         ("515x511",      515, 511, 1, 0.3,     True),
         ("all_invalid",  9,   31,  1, 1.0,     True),
         # general cameras (scenes.CAMERAS): under a turn about y, c2w[0][1], [1][0], [1][2], [2][1] are 0 and c2w[1][1] is 1
         ("skew23",       37,  23,  3, 0.1,     "skew23"),
         ("skew140",      64,  48,  1, 0.3,     "skew140"),
         ("roll90",       37,  23,  1, 0.1,     "roll90"),
         ("pitch17",      7,   5,   3, 0.0,     "pitch17")]


def _w2c(tilted):
    """False: the identity; True: the turn about y; a name: that camera of scenes.CAMERAS"""
    if not tilted:
        return torch.eye(4)
    import scenes
    return torch.tensor(np.asarray(scenes.tilted_w2c() if tilted is True else scenes.CAMERAS[tilted])).float()


def _frame(H, W, invalid, seed):
    g = torch.Generator().manual_seed(seed)
    depth = torch.rand(1, H, W, generator=g) * 5.5 + 0.5
    if invalid > 0:
        u = torch.rand(1, H, W, generator=g)
        depth = torch.where(u < invalid / 2, torch.zeros(()), depth)                        # half of the holes are zeros,
        depth = torch.where((u >= invalid / 2) & (u < invalid), -depth, depth)              # half negative
    color = torch.rand(3, H, W, generator=g)
    f = 0.9 * W + 3.0
    intrinsics = torch.tensor([[f, 0.0, (W - 1) / 2.0 + 0.25], [0.0, 1.1 * f, (H - 1) / 2.0 - 0.25], [0.0, 0.0, 1.0]])
    return color.cuda(), depth.cuda(), intrinsics.cuda()


def _restatement(color, depth, intrinsics, c2w, S, dtype):
    """get_pointcloud + initialize_params + scene_radius in `dtype`, on the device, in the reference's order"""
    color, depth, intrinsics, c2w = color.to(dtype), depth.to(dtype), intrinsics.to(dtype), c2w.to(dtype)
    width, height = color.shape[2], color.shape[1]
    CX, CY, FX, FY = intrinsics[0][2], intrinsics[1][2], intrinsics[0][0], intrinsics[1][1]
    x_grid, y_grid = torch.meshgrid(torch.arange(width, device=depth.device).to(dtype), torch.arange(height, device=depth.device).to(dtype),
                                    indexing='xy')
    xx = ((x_grid - CX) / FX).reshape(-1)
    yy = ((y_grid - CY) / FY).reshape(-1)
    depth_z = depth[0].reshape(-1)
    pts_cam = torch.stack((xx * depth_z, yy * depth_z, depth_z), dim=-1)
    pts4 = torch.cat((pts_cam, torch.ones(height * width, 1, device=depth.device, dtype=dtype)), dim=1)
    pts = (c2w @ pts4.T).T[:, :3]
    scale_gaussian = depth_z / ((FX + FY) / 2)
    mean3_sq_dist = scale_gaussian ** 2
    cols = torch.permute(color, (1, 2, 0)).reshape(-1, 3)
    mask = (depth > 0).reshape(-1)
    pts, cols, mean3_sq_dist = pts[mask], cols[mask], mean3_sq_dist[mask]
    n = pts.shape[0]
    rots = torch.zeros(n, 4, device=depth.device, dtype=dtype)
    rots[:, 0] = 1
    return dict(count=n, means3D=pts, rgb=cols, log_scales=torch.tile(torch.log(torch.sqrt(mean3_sq_dist))[..., None], (1, S)),
                unnorm_rotations=rots, logit_opacities=torch.zeros(n, 1, device=depth.device, dtype=dtype),
                scene_radius=torch.max(depth) / RATIO)


def _run(color, depth, intrinsics, w2c_dev, S, capacity=None):
    from hsr_utils import slam
    M, means, rgb, ls, rots, opac, radius = slam.map_init_frame(color, depth, intrinsics, w2c_dev, RATIO, S, capacity=capacity)
    return dict(count=M, means3D=means, rgb=rgb, log_scales=ls, unnorm_rotations=rots, logit_opacities=opac, scene_radius=radius[0])


def _compare(name, got, ref32, ref64, rows=None):
    rows = got["count"] if rows is None else rows
    assert got["count"] == ref32["count"]
    for k in ("rgb", "unnorm_rotations", "logit_opacities"):
        assert got[k].shape == ref32[k][:rows].shape and torch.equal(got[k], ref32[k][:rows]), (name, k)
    assert torch.equal(got["scene_radius"], ref32["scene_radius"]), (name, float(got["scene_radius"]), float(ref32["scene_radius"]))
    for k in ("means3D", "log_scales"):
        assert got[k].shape == ref32[k][:rows].shape, (name, k)
        if rows == 0:
            continue
        exact = torch.equal(got[k], ref32[k][:rows])
        d_kernel = float((got[k].double() - ref64[k][:rows]).abs().max())
        d_torch = float((ref32[k][:rows].double() - ref64[k][:rows]).abs().max())
        print("map_init %-12s %-10s bit-equal to the fp32 restatement: %s   |kernel - f64| %.3e   |fp32 restatement - f64| %.3e"
              % (name, k, exact, d_kernel, d_torch))
        assert exact or d_kernel <= 2.0 * d_torch, (name, k, d_kernel, d_torch)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_map_init_matches_the_restatement(case):
    name, H, W, S, invalid, tilted = case
    color, depth, intrinsics = _frame(H, W, invalid, seed=H * 1000 + W)
    w2c = _w2c(tilted).cuda()
    c2w = torch.inverse(w2c)                                       # what the wrapper hands the kernel (scripts/hierslam.py:167)
    ref32 = _restatement(color, depth, intrinsics, c2w, S, torch.float32)
    ref64 = _restatement(color, depth, intrinsics, c2w, S, torch.float64)
    got = _run(color, depth, intrinsics, w2c, S)
    again = _run(color, depth, intrinsics, w2c, S)
    expected = 0 if invalid >= 1.0 else int((depth > 0).sum())
    assert got["count"] == expected and (invalid >= 1.0 or 0 < expected <= H * W)
    if 0.0 < invalid < 1.0:
        assert expected < H * W
    _compare(name, got, ref32, ref64)
    for k, v in got.items():                                       # two calls: the same bits
        assert v == again[k] if k == "count" else torch.equal(v, again[k]), k


def test_capacity_below_the_count():
    """capacity < M: the first `capacity` rows are written, the count is still M, and nothing is written past the buffers"""
    from diff_gaussian_rasterization import _abi
    H, W, S = 37, 23, 3
    color, depth, intrinsics = _frame(H, W, 0.1, seed=5)
    w2c = _w2c(True).cuda()
    c2w = torch.inverse(w2c).contiguous()
    ref32 = _restatement(color, depth, intrinsics, c2w, S, torch.float32)
    ref64 = _restatement(color, depth, intrinsics, c2w, S, torch.float64)
    M = ref32["count"]
    cap = 300                                                      # ends inside the second 256-pixel block
    assert 256 < cap < M
    got = _run(color, depth, intrinsics, w2c, S, capacity=cap)
    assert got["count"] == M and got["means3D"].shape == (cap, 3) and got["log_scales"].shape == (cap, S)
    _compare("capacity", got, ref32, ref64, rows=cap)
    # the raw call with guard rows behind the capacity: they keep their fill
    lib = _abi.lib
    K = intrinsics.cpu()
    guard = 64
    o = dict(dtype=torch.float32, device="cuda")
    bufs = [torch.full((cap + guard, c), -7.0, **o) for c in (3, 3, S, 4, 1)]
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    radius = torch.zeros(1, **o)
    sc = torch.empty(int(lib.hsr_map_init_scratch_bytes(H, W)), dtype=torch.uint8, device="cuda")
    _abi.call(lib.hsr_map_init_frame, "hsr_map_init_frame", depth.device, H, W, depth.data_ptr(), color.data_ptr(), float(K[0, 0]), float(K[1, 1]),
              float(K[0, 2]), float(K[1, 2]), c2w.data_ptr(), RATIO, cap, S, count.data_ptr(), *[b.data_ptr() for b in bufs], radius.data_ptr(),
              sc.data_ptr(), sc.numel())
    assert int(count) == M
    for b, k in zip(bufs, ("means3D", "rgb", "log_scales", "unnorm_rotations", "logit_opacities")):
        assert torch.equal(b[:cap], got[k]) and bool((b[cap:] == -7.0).all()), k
    # capacity 0 counts only, with no row buffers at all; a too-small scratch is refused
    count.zero_()
    rc = lib.hsr_map_init_frame(H, W, depth.data_ptr(), color.data_ptr(), 1.0, 1.0, 0.0, 0.0, c2w.data_ptr(), RATIO, 0, 1, count.data_ptr(),
                                None, None, None, None, None, None, sc.data_ptr(), sc.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and int(count) == M
    rc = lib.hsr_map_init_frame(H, W, depth.data_ptr(), color.data_ptr(), 1.0, 1.0, 0.0, 0.0, c2w.data_ptr(), RATIO, 0, 1, count.data_ptr(),
                                None, None, None, None, None, None, sc.data_ptr(), 8, None)
    assert rc == _abi.HSR_ERR_BUFFER_TOO_SMALL and b"scratch too small" in lib.hsr_last_error()
    rc = lib.hsr_map_init_frame(H, W, depth.data_ptr(), color.data_ptr(), 1.0, 1.0, 0.0, 0.0, c2w.data_ptr(), RATIO, 0, 2, count.data_ptr(),
                                None, None, None, None, None, None, sc.data_ptr(), sc.numel(), None)
    assert rc == -1 and b"S=2" in lib.hsr_last_error()


@pytest.mark.parametrize("num_semantic,distribution,S", [(None, "isotropic", 1), (None, "anisotropic", 3), ([2, 2], "isotropic", 1)])
def test_initialize_first_timestep_keys_and_shapes(num_semantic, distribution, S):
    """the public entry: keys, shapes and leaf Parameters of initialize_params / initialize_semantic_params, zeroed bookkeeping, scene_radius"""
    from hsr_utils import initialize_first_timestep
    H, W, frames = 64, 48, 6
    color, depth, intrinsics = _frame(H, W, 0.3, seed=11)
    w2c = _w2c(True).cuda()
    ref32 = _restatement(color, depth, intrinsics, torch.inverse(w2c), S, torch.float32)
    torch.manual_seed(3)
    params, variables = initialize_first_timestep(color, depth, intrinsics, w2c, frames, RATIO, "projective", distribution, num_semantic)
    N = ref32["count"]
    keys = ["means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales"] + (["semantic"] if num_semantic else []) \
        + ["cam_unnorm_rots", "cam_trans"]
    assert list(params) == keys
    shapes = dict(means3D=(N, 3), rgb_colors=(N, 3), unnorm_rotations=(N, 4), logit_opacities=(N, 1), log_scales=(N, S), semantic=(N, 4),
                  cam_unnorm_rots=(1, 4, frames), cam_trans=(1, 3, frames))
    for k, p in params.items():
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf and p.is_contiguous() and p.dtype == torch.float32, k
        assert tuple(p.shape) == shapes[k], k
    assert torch.equal(params["rgb_colors"].detach(), ref32["rgb"]) and torch.equal(params["unnorm_rotations"].detach(), ref32["unnorm_rotations"])
    assert torch.equal(params["cam_trans"].detach(), torch.zeros(1, 3, frames, device="cuda"))
    assert torch.equal(params["cam_unnorm_rots"].detach()[0], torch.tensor([1.0, 0, 0, 0], device="cuda")[:, None].expand(4, frames))
    if num_semantic:
        torch.manual_seed(3)
        assert torch.equal(params["semantic"].detach(), torch.rand((N, 4), device="cuda"))      # the reference's draw (:376)
    assert sorted(variables) == ["denom", "max_2D_radius", "means2D_gradient_accum", "scene_radius", "timestep"]
    for k in ("denom", "max_2D_radius", "means2D_gradient_accum", "timestep"):
        assert variables[k].shape == (N,) and variables[k].dtype == torch.float32 and not variables[k].any(), k
    assert variables["scene_radius"].dim() == 0 and torch.equal(variables["scene_radius"], ref32["scene_radius"])
