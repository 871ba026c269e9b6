"""CPU checks of the warp loss's yardstick (tests/warp_reference.py, the float64 restatement the GPU tests compare the HIP kernels
with): pinned to golden G21 (the reference's own torch code, tests/golden/make_golden_warp.py) where the reference has a torch
form, and to known answers of view_selection_kernel.cu:19-72 where it has none.  Plus the module's schedule and shape rules."""
import math
import types

import numpy as np
import pytest
import torch

import warp_reference as WR

F64 = torch.float64


@pytest.fixture(scope="module")
def g21(golden):
    return {k: torch.from_numpy(v) if v.ndim else v for k, v in golden("g21_warp").items()}


def test_projection_matches_reference_torch_twin(g21):
    """proj_points2grid + camera.world2cam (warp_loss.py:232-269) for every (camera, point): grid, neighbour direction and depth."""
    N, B = g21["rts"].shape[0], g21["x"].shape[0]
    H, W = int(g21["H"]), int(g21["W"])
    views = torch.arange(N)[None, :].expand(B, N)
    grid, depth, origin, direction = WR.project(g21["x"], g21["ks"], g21["rts"], views)
    front = g21["far"].T > 0
    assert front.float().mean() > 0.9
    gn = g21["grid_norm"].permute(1, 0, 2)
    want = torch.stack([(gn[..., 0] + 1) / 2 * (W - 1), (gn[..., 1] + 1) / 2 * (H - 1)], -1) - 0.5
    np.testing.assert_allclose(grid[front].numpy(), want[front].numpy(), rtol=1e-10, atol=1e-9)
    np.testing.assert_allclose(depth.numpy(), g21["far"].T.numpy(), rtol=1e-12, atol=1e-12)
    # (the torch twin divides all three camera-space components by z + 1e-8; the CUDA kernel, which the library follows, sets the
    # third to 1: they differ by 1e-8 / z)
    np.testing.assert_allclose(direction[front].numpy(), g21["nei_dirs"].permute(1, 0, 2)[front].numpy(), rtol=0, atol=2e-8)
    # neighbour origin = the camera centre: the point lies on the neighbour ray origin + s * direction, s = camera-space depth
    np.testing.assert_allclose((origin + depth[..., None] * direction)[front].numpy(),
                               g21["x"][:, None, :].expand(B, N, 3)[front].numpy(), rtol=0, atol=1e-8)


def test_sample_color_matches_reference(g21):
    """sample_neighbor_color (warp_loss.py:441-521), negative sub-pixel grids and partial occlusions included, and its gradient
    w.r.t. grid."""
    grid = g21["grid"].clone().requires_grad_(True)
    assert (grid.detach() < 0).any() and (grid.detach() > -0.5).all()
    color, valid = WR.sample_color(g21["images"], g21["occlusions"], grid, g21["views"], g21["valid_in"])
    assert torch.equal(valid, g21["valid"])
    assert (g21["valid_in"] & ~g21["valid"]).any()          # the occlusions removed some slots
    np.testing.assert_allclose(color.detach().numpy(), g21["color"].numpy(), rtol=1e-12, atol=1e-12)
    (color * g21["wgt"]).sum().backward()
    np.testing.assert_allclose(grid.grad.numpy(), g21["grad_grid"].numpy(), rtol=1e-10, atol=1e-12)


def test_scores_loss_and_warming(g21):
    np.testing.assert_allclose(WR.soft_vis(g21["depth_diff"], float(g21["alpha"]), float(g21["voxel_size"])).numpy(),
                               g21["vis"].numpy(), rtol=1e-12)
    np.testing.assert_allclose(WR.soft_diffuse(g21["specular"], float(g21["gamma"])).numpy(), g21["diffuse_score"][:, 0].numpy(),
                               rtol=1e-12)
    c1, c2, score = g21["c1"], g21["c2"], g21["score"][..., 0]
    # compute_loss on clamp(dif + spec, 0, 1): split c1 (in [0, 1]) into a diffuse and a specular half
    loss = WR.compute_loss(c1[:, 0] * 0.5, c1[:, 0] * 0.5, c2, score, c1.shape[0])
    ref = (((c1[:, :1] - c2) ** 2).mean(-1) * score).mean()
    np.testing.assert_allclose(float(loss), float(ref), rtol=1e-12)
    want = (((c1 - c2) ** 2).mean(-1, keepdim=True) * g21["score"]).mean()
    np.testing.assert_allclose(float(want), float(g21["loss"]), rtol=1e-12)
    from scanerf_amd.warp import warp_weight_warming
    got = [warp_weight_warming(1.5, int(s)) for s in g21["steps"]]
    np.testing.assert_allclose(got, g21["warm"], rtol=0, atol=0)


# ---- view costs: known answers of computeViewcost_kernel ------------------------------------------------------------------
def _camera(c, look, f=50.0, W=64, H=48):
    z = look / np.linalg.norm(look)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    rt = np.concatenate([R, (-R @ c)[:, None]], 1)
    return torch.tensor(rt)[None], torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], dtype=F64)[None], H, W


def _cost(o, d, p, cam):
    rt, k, H, W = cam
    t = lambda v: torch.tensor([list(map(float, v))], dtype=F64)
    return float(WR.view_costs(t(o), t(d), t(p), k, rt, H, W)[0, 0])


def test_view_cost_behind_the_camera_is_one():
    cam = _camera(np.array([0.0, 0, 0]), np.array([0.0, 0, 1]))
    assert _cost([0, 0, -5], [0, 0, 1], [0, 0, -1], cam) == 1.0
    assert _cost([0, 0, -5], [0, 0, 1], [0, 0, 0.0005], cam) == 1.0   # uv.z <= 0.001


def test_view_cost_on_the_image_border_is_one():
    rt, k, H, W = _camera(np.array([0.0, 0, 0]), np.array([0.0, 0, 1]))
    # x = f X / Z + W/2 = 0 exactly (the open interval excludes the border), and = W - 1
    z = 2.0
    p0 = [-(W / 2) * z / 50.0, 0.0, z]
    p1 = [(W - 1 - W / 2) * z / 50.0, 0.0, z]
    assert _cost([0, 0, -3], [0, 0, 1], p0, (rt, k, H, W)) == 1.0
    assert _cost([0, 0, -3], [0, 0, 1], p1, (rt, k, H, W)) == 1.0
    p2 = [(W - 1.01 - W / 2) * z / 50.0, 0.0, z]                        # just inside
    assert _cost([0, 0, -3], [0, 0, 1], p2, (rt, k, H, W)) < 1.0


def test_view_cost_head_on_is_zero():
    """A neighbour camera AT the ray's origin, seeing the point straight along the ray: angle cost 0, distance cost
    max(0, 1 - |p - o| / |p - c|) = 0."""
    c = np.array([0.3, -0.2, -4.0])
    p = np.array([0.1, 0.1, 0.5])
    cam = _camera(c, p - c)
    assert abs(_cost(list(c), list(2.5 * (p - c)), list(p), cam)) < 1e-12


def test_view_cost_formula_off_axis():
    """0.9 (1 - cos angle) + 0.1 max(0, 1 - |p - o| / |p - c|) for a neighbour 30 degrees off the ray, nearer to the point."""
    p = np.array([0.0, 0.0, 0.0])
    o = np.array([0.0, 0.0, -4.0])
    a = math.radians(30)
    c = 2.0 * np.array([math.sin(a), 0.0, -math.cos(a)])
    cam = _camera(c, p - c)
    want = 0.9 * (1 - math.cos(a)) + 0.1 * max(0.0, 1 - 4.0 / 2.0)
    assert abs(_cost(list(o), [0, 0, 1], list(p), cam) - want) < 1e-12
    c = 8.0 * np.array([math.sin(a), 0.0, -math.cos(a)])
    want = 0.9 * (1 - math.cos(a)) + 0.1 * (1 - 4.0 / 8.0)
    assert abs(_cost(list(o), [0, 0, 1], list(p), _camera(c, p - c)) - want) < 1e-12


def test_selection_keeps_lowest_and_breaks_ties_by_index():
    costs = torch.tensor([[0.5, 0.1, 0.1, 1.0, 0.05, 0.1], [1.0, 1.0, 0.2, 0.17, 0.176, 0.3]], dtype=F64)
    v, c, valid = WR.select(costs, 3)
    assert v.tolist() == [[4, 1, 2], [3, 4, 2]]
    assert valid.tolist() == [[True, True, True], [True, True, False]]
    v, c, valid = WR.select(costs, 3, ray_valid=torch.tensor([True, False]))
    assert valid[1].tolist() == [False, False, False]


def test_warp_loss_module_rules():
    """K = min(top_k, N) (topk(k=10) raises in the reference when a tile sees fewer cameras); the LossItem schedule."""
    from scanerf_amd.warp import WarpLoss
    cams = types.SimpleNamespace(ks=torch.eye(3, dtype=torch.float32).expand(7, 3, 3), get_rts=None)
    imgs = torch.zeros(7, 8, 9, 3, dtype=torch.float32)
    w = WarpLoss(cams, imgs, voxel_size=0.1)
    assert w.K == 7 and (w.N, w.H, w.W) == (7, 8, 9)
    assert WarpLoss(cams, imgs, voxel_size=0.1, top_k=4).K == 4
    w = WarpLoss(cams, imgs, voxel_size=0.1, weight=2.0, start_step=100)
    assert w.scale(100) == 0.0 and w.scale(5100) == 1.0 and w.scale(20000) == 2.0
    assert WarpLoss(cams, imgs, voxel_size=0.1, weight=2.0, warming=False).scale(1) == 2.0
    with pytest.raises(ValueError):
        WarpLoss(cams, imgs)
    with pytest.raises(ValueError):
        WarpLoss(cams, imgs[:3], voxel_size=0.1)
    with pytest.raises(ValueError):
        WarpLoss(cams, imgs, occlusions=torch.ones(7, 8, 8, dtype=torch.bool), voxel_size=0.1)
