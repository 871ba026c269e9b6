"""Golden vector G21 from the reference's warp loss (warp_loss.py, criterions.py).

    python tests/golden/make_golden_warp.py          (build container only: the reference checkout must exist)

G21  the torch parts of warp_loss.WarpLoss, run by the reference's own code on the CPU in float64:
     proj_points2grid + camera.world2cam (warp_loss.py:232-269: the torch twin of proj2neighbor_forward) -> grid (normalised to
     [-1, 1]), neighbour directions, camera-space depth of every (camera, point);
     sample_neighbor_color (warp_loss.py:441-521) with its autograd to grid -> colours, occlusion-masked valid flags, dL/dgrid of
     sum(colour * wgt); soft_vis / soft_diffuse (alpha = 10, gamma = 20), compute_loss, criterions.warp_weight_warming_func.
     Fixture: 12 cameras on a ring around the origin, a 40 x 32 image, 500 points, grids with negative sub-pixel coordinates,
     partial occlusions.  The view costs have no torch form in the reference (computeViewcost is CUDA-only): tests/test_warp_cpu.py
     checks them by known answers instead.
Only DATA is written (inputs + the reference's outputs); nothing here runs on the GPU box."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _stub_modules  # noqa: E402

sys.dont_write_bytecode = True

N, H, W, B, K = 12, 32, 40, 500, 4


def ring_cameras(n, radius=3.0, f=30.0):
    """World-to-camera [n,3,4] of cameras on a ring in the y = 0.3 plane looking at the origin, and their intrinsics [n,3,3]."""
    rts, ks = [], []
    for i in range(n):
        a = 2 * np.pi * i / n
        c = np.array([radius * np.cos(a), 0.3 + 0.1 * np.sin(3 * a), radius * np.sin(a)])
        z = -c / np.linalg.norm(c)
        x = np.cross(np.array([0.0, 1.0, 0.0]), z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z])
        rts.append(np.concatenate([R, (-R @ c)[:, None]], 1))
        ks.append([[f, 0, W / 2 + 0.3 * i], [0, f * 1.02, H / 2 - 0.2 * i], [0, 0, 1]])
    return np.array(rts), np.array(ks, dtype=np.float64)


def main():
    _stub_modules()
    cu = sys.modules["cuda"]
    for n in ["computeViewcost", "grid_sample_forward_cuda", "grid_sample_backward_cuda", "gaussian_grid_sample_forward_cuda",
              "gaussian_grid_sample_backward_cuda", "grid_sample_bool_cuda", "proj2neighbor_forward", "proj2neighbor_backward"]:
        setattr(cu, n, getattr(cu, "ray_aabb_intersection"))
    tv = types.ModuleType("torchvision")          # warp_loss.py:6 (used by build_pyramid only)
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tv.transforms
    sys.modules["tools"].utils = types.ModuleType("tools.utils")
    sys.modules["tools.utils"] = sys.modules["tools"].utils
    for m in ("mono_loss",):                      # criterions.py imports it; its classes are not used here
        mm = types.ModuleType(m)
        mm.DepthConsistencyLoss = mm.DepthSmoothLoss = object
        sys.modules[m] = mm
    sys.path.insert(0, REF)
    import criterions  # noqa
    import warp_loss  # noqa

    g = torch.Generator().manual_seed(21)
    rts, ks = ring_cameras(N)
    rts, ks = torch.from_numpy(rts), torch.from_numpy(ks)
    x = (torch.rand(B, 3, generator=g, dtype=torch.float64) - 0.5) * 1.2
    images = torch.rand(N, H, W, 3, generator=g, dtype=torch.float64)
    occl = torch.rand(N, H, W, generator=g) > 0.25

    wl = object.__new__(warp_loss.WarpLoss)
    wl.H, wl.W, wl.z_thresh, wl.device = H, W, 0, "cpu"
    wl.poses = types.SimpleNamespace(ks=ks)
    wl.images = images
    wl.alpha, wl.gamma, wl.voxel_size = 10.0, 20.0, 0.05
    wl.topK = K

    grid_n, dirs, far = wl.proj_points2grid(x, rts)          # [N,B,1,2], [N,B,3], [N,B]

    # sample_neighbor_color: grids inside the image's bilinear support, a tenth of them with a negative sub-pixel coordinate
    gx = torch.rand(B, K, generator=g, dtype=torch.float64) * (W - 2.02) - 0.49
    gy = torch.rand(B, K, generator=g, dtype=torch.float64) * (H - 2.02) - 0.49
    neg = torch.rand(B, K, generator=g) < 0.1
    gx = torch.where(neg, -torch.rand(B, K, generator=g, dtype=torch.float64) * 0.49, gx)
    gy = torch.where(torch.rand(B, K, generator=g) < 0.1, -torch.rand(B, K, generator=g, dtype=torch.float64) * 0.49, gy)
    grid = torch.stack([gx, gy], -1).requires_grad_(True)
    views = torch.randint(0, N, (B, K), generator=g).int()
    valid_in = torch.rand(B, K, generator=g) < 0.9
    color, valid = wl.sample_neighbor_color(grid, views, valid_in, occl)
    wgt = torch.randn(B, K, 3, generator=g, dtype=torch.float64)
    (color * wgt).sum().backward()

    depth_diff = torch.rand(B, 1, generator=g, dtype=torch.float64) * 0.3
    spec = torch.rand(B, 3, generator=g, dtype=torch.float64) * 0.2
    c1, c2 = torch.rand(B, K, 3, generator=g, dtype=torch.float64), torch.rand(B, K, 3, generator=g, dtype=torch.float64)
    score = torch.rand(B, K, 1, generator=g, dtype=torch.float64)
    steps = np.array([-5, 0, 1, 2500, 9999, 10000, 25000])

    out = dict(
        rts=rts, ks=ks, H=H, W=W, x=x, grid_norm=grid_n[:, :, 0, :], nei_dirs=dirs, far=far,
        images=images, occlusions=occl, grid=grid.detach(), views=views, valid_in=valid_in, color=color.detach(), valid=valid,
        wgt=wgt, grad_grid=grid.grad, depth_diff=depth_diff, vis=wl.soft_vis(depth_diff), specular=spec,
        diffuse_score=wl.soft_diffuse(spec), alpha=10.0, gamma=20.0, voxel_size=0.05, c1=c1, c2=c2, score=score,
        loss=wl.compute_loss(c1, c2, score), steps=steps,
        warm=np.array([criterions.warp_weight_warming_func(1.5, int(s)) for s in steps]))
    out = {k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, "g21_warp.npz"), **out)
    print("wrote g21_warp", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
