"""Golden vector G22 from the reference's monocular losses (mono_loss.py, criterions.py).

    python tests/golden/make_golden_mono.py          (build container only: the reference checkout must exist)

G22  mono_loss.DepthConsistencyLoss and mono_loss.DepthSmoothLoss, run by the reference's own code on the CPU in float64 on the
     batch layout of tile.py:902-948 (view-major [num_camera, Bc], the same 2x2-patch pixel set in every view, pixel_locs (x, y)),
     with their autograd gradients w.r.t. rendered_depth; and criterions.LossItem's schedule (depth / smooth_weight_decay_func,
     start < step < end) at chosen steps.
     tools/utils.py cannot be imported here (it needs cv2 and imageio): its Mask_MSELoss is taken from the file with `ast` (that
     one function definition, compiled into a stub tools.utils module); nothing of it is written out.  warp_loss (imported by
     criterions.py, unused by LossItem) is a stub module.
     Cases:
       main    8 views x 128 rays: view 0 has exactly one valid ray (det = 0), view 1 none, views 2 and 3 depths 50 +- 1 (2 %),
               patches whose normals fail the 0.9 test, patches with one masked ray;
       nopatch 2 views x 16 rays, every patch fails the normal test: the reference's smoothness loss is NaN;
       empty   2 views x 16 rays, no valid ray: the reference's depth loss is None (stored as has_depth = False), smoothness NaN.
     Inputs are rounded to float32 first (the GPU kernels read float32), so a float32 cast of them is exact.
Only DATA is written (inputs + the reference's outputs); nothing here runs on the GPU box."""
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _stub_modules  # noqa: E402

sys.dont_write_bytecode = True
F64 = torch.float64


def mask_mse_from_reference():
    """tools/utils.py's Mask_MSELoss, compiled from its own definition (the module itself needs cv2 / imageio)."""
    src = open(os.path.join(REF, "tools", "utils.py")).read()
    fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "Mask_MSELoss")
    ns = {"torch": torch}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "utils.py", "exec"), ns)
    return ns["Mask_MSELoss"]


def f32(t):
    return t.float().to(F64)


def patch_pixels(g, num_patch, H, W):
    """tile.py:913-921: top-left corners from two permutations, utils.get_ray_idx's 2x2 order -> pixel_locs [Bc, 2] (x, y)."""
    px = torch.randperm(W - 2, generator=g)[:num_patch]
    py = torch.randperm(H - 2, generator=g)[:num_patch]
    idx = (py * W + px)[:, None, None] + (torch.arange(2)[None, :] + (torch.arange(2) * W)[:, None])[None]
    idx = idx.reshape(-1)
    return torch.stack([idx % W, idx // W], -1)


def make_case(g, N, num_patch, H, W, kind):
    Bc = 4 * num_patch
    ks = torch.zeros(N, 3, 3, dtype=F64)
    for v in range(N):
        ks[v] = torch.tensor([[40.0 + v, 0.0, W / 2 + 0.3 * v], [0.0, 41.0 - 0.5 * v, H / 2 - 0.2 * v], [0.0, 0.0, 1.0]])
    ks = f32(ks)
    locs2 = patch_pixels(g, num_patch, H, W)
    # a plane-ish surface per view plus noise; views 2, 3 of the main case at 50 +- 1
    base = 2.0 + 3.0 * torch.rand(N, 1, generator=g, dtype=F64)
    depth = base + 0.5 * torch.rand(N, Bc, generator=g, dtype=F64)
    if kind == "main":
        depth[2:4] = 50.0 + (2.0 * torch.rand(2, Bc, generator=g, dtype=F64) - 1.0)
    a = 0.5 + torch.rand(N, 1, generator=g, dtype=F64)
    b = torch.rand(N, 1, generator=g, dtype=F64) - 0.5
    # the monocular maps [N,H,W(,3)], read at the batch's pixels (overlapping patches share pixels, as in the reference)
    pix = locs2[:, 1] * W + locs2[:, 0]
    mono_map = torch.zeros(N, H * W, dtype=F64)
    mono_map[:, pix] = a * depth + b + 0.05 * torch.randn(N, Bc, generator=g, dtype=F64)
    mono = mono_map[:, pix]
    # normals: one per patch, jittered per ray; some patches random (fail the 0.9 test)
    pn = torch.nn.functional.normalize(torch.randn(N, num_patch, 1, 3, generator=g, dtype=F64) + torch.tensor([0, 0, -2.0]), dim=-1)
    normal = pn + 0.05 * torch.randn(N, num_patch, 4, 3, generator=g, dtype=F64)
    bad = torch.rand(N, num_patch, generator=g) < (1.0 if kind == "nopatch" else 0.2)
    normal[bad] = torch.randn(int(bad.sum()), 4, 3, generator=g, dtype=F64)
    normal_map = torch.zeros(N, H * W, 3, dtype=F64)
    normal_map[:, pix] = torch.nn.functional.normalize(normal, dim=-1).reshape(N, Bc, 3)
    normal = normal_map[:, pix]
    mask = torch.ones(N, Bc, dtype=torch.bool)
    if kind == "main":
        mask = torch.rand(N, Bc, generator=g) > 0.1          # scattered masked rays: patches with one masked ray
        mask[0] = False
        mask[0, 5] = True                                     # view 0: exactly one valid ray
        mask[1] = False                                       # view 1: none
    elif kind == "empty":
        mask[:] = False
    return dict(ks=ks, pixel_locs=locs2, depth=f32(depth), mono_depth=f32(mono), mono_normal=f32(normal), mask=mask, H=H, W=W)


def run_reference(mono_loss, c):
    N, Bc = c["depth"].shape
    depth = c["depth"].clone()[..., None].requires_grad_(True)
    mask = c["mask"][..., None]
    out = {}
    ld = mono_loss.DepthConsistencyLoss()(depth, c["mono_depth"][..., None], mask)
    out["has_depth"] = ld is not None
    if ld is not None:
        ld.backward()
        out["loss_depth"], out["grad_depth"] = ld.detach(), depth.grad[..., 0].clone()
    else:
        out["loss_depth"], out["grad_depth"] = torch.tensor(0.0, dtype=F64), torch.zeros(N, Bc, dtype=F64)
    depth.grad = None
    block = types.SimpleNamespace(poses=types.SimpleNamespace(ks=c["ks"]), num_camera=N)
    pixel_locs = c["pixel_locs"][None].repeat(N, 1, 1)
    ls = mono_loss.DepthSmoothLoss(None, block)(pixel_locs, depth, c["mono_normal"], mask)
    out["loss_smooth"] = ls.detach()
    if torch.isfinite(ls):
        ls.backward()
        out["grad_smooth"] = depth.grad[..., 0].clone()
    else:
        out["grad_smooth"] = torch.full((N, Bc), float("nan"), dtype=F64)
    return out


def main():
    _stub_modules()
    ut = types.ModuleType("tools.utils")
    ut.Mask_MSELoss = mask_mse_from_reference()
    sys.modules["tools"].utils = ut
    sys.modules["tools.utils"] = ut
    sys.modules["warp_loss"] = types.ModuleType("warp_loss")
    sys.path.insert(0, REF)
    import criterions  # noqa
    import mono_loss  # noqa

    g = torch.Generator().manual_seed(22)
    out = {}
    for kind, N, num_patch in (("main", 8, 32), ("nopatch", 2, 4), ("empty", 2, 4)):
        c = make_case(g, N, num_patch, 40, 48, kind)
        r = run_reference(mono_loss, c)
        for k, v in {**c, **r}.items():
            out[f"{kind}_{k}"] = v

    # LossItem's schedule: the weight the term is added with at each step (0 = not added)
    steps = np.array([0, 1, 499, 500, 501, 30000, 30500, 39999, 40000, 40001])
    one = lambda **kw: torch.tensor(1.0, dtype=F64)
    for name, fn, w in (("depth", criterions.depth_weight_decay_func, 0.01), ("smooth", criterions.smooth_weight_decay_func, 0.001)):
        for start in (0, 500):
            item = criterions.LossItem(name, one, w, start, end_step=40000, decay_func=fn)
            out[f"sched_{name}_{start}"] = np.array([float(item(0, int(s))) for s in steps])
    out["sched_steps"] = steps
    out = {k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, "g22_mono.npz"), **out)
    print("wrote g22_mono", {k: v.shape for k, v in out.items()})
    print({k: float(v) for k, v in out.items() if k.endswith("loss_depth") or k.endswith("loss_smooth")})


if __name__ == "__main__":
    main()
