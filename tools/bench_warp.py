"""Cost of the multi-view warp term (scanerf_amd.warp, csrc/warp.hip) on the reference's shipped iteration: T = 2^24, 16 384 rays,
foreground + T_left * background (128 + 128 samples), pose refinement (train_step_fgbg(pose_grads=True), bench.py's
reference_default leg) -- timed with the warp term off and on.

    python tools/bench_warp.py [--steps 8] [--warmup 2] [--cameras 64]

The rays come from a block of cameras close enough together that every ray has its 10 neighbour candidates (cost <= 0.176); the
output reports how many slots were valid and how many neighbour rays the visibility render traced.  One JSON line.  For the
per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_warp.py`."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def camera_block(n, H, W, f, dev):
    """n cameras on a jittered grid in the z = -3.5 plane, 0.8 m across, looking along +z (into the tile)."""
    from scanerf_amd import cameras as CM
    side = int(round(n ** 0.5))
    g = torch.Generator().manual_seed(3)
    c2w = []
    for i in range(n):
        x, y = (i % side) / max(side - 1, 1) - 0.5, (i // side) / max(side - 1, 1) - 0.5
        c = torch.tensor([0.8 * x, 0.8 * y, -3.5]) + 0.02 * torch.randn(3, generator=g)
        c2w.append(torch.cat([torch.eye(3), c[:, None]], 1))
    ks = torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1.0]]).expand(n, 3, 3)
    return CM.CameraSet(ks, torch.stack(c2w), dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cameras", type=int, default=64)
    ap.add_argument("--rays", type=int, default=16384)
    ap.add_argument("--log2-T", type=int, default=24)
    ap.add_argument("--samples", type=int, default=128)
    args = ap.parse_args()
    import scanerf_amd  # noqa
    from scanerf_amd import tile_model as tm
    from scanerf_amd.warp import WarpLoss
    dev = "cuda:0"
    H, W, S, B = 300, 400, args.samples, args.rays
    cams = camera_block(args.cameras, H, W, 200.0, dev)
    g = torch.Generator(device=dev).manual_seed(24)
    images = torch.rand(args.cameras, H, W, 3, device=dev, generator=g)
    locs = torch.stack([torch.randint(0, args.cameras, (B,), device=dev, generator=g),
                        torch.randint(0, W, (B,), device=dev, generator=g), torch.randint(0, H, (B,), device=dev, generator=g)], 1).int()
    tg = torch.rand(B, 3, device=dev, generator=g)
    step0 = 20000
    res = {}
    for leg in ("off", "on"):
        m = tm.TileModel([-4.0, -4, -4], [8, 8, 8], dev, log2_T=args.log2_T, seed=24, sampler_log2dim=4)
        opt = torch.optim.Adam(m.decoder.parameters(), lr=1e-3, betas=(0.9, 0.99), eps=1e-15)
        warp = None
        if leg == "on":
            warp = WarpLoss(cams, images, None, voxel_size=float((m.bbox_size / 2048).max()), start_step=0)
        ro, rd = (x.detach().contiguous() for x in cams.get_rays(locs))

        def step(i, timer=None):
            cams.se3_refine.grad = None
            loss, g_o, g_d = tm.train_step_fgbg(m, opt, ro, rd, tg, S, S, step0 + i, pose_grads=True, timer=timer,
                                                **({"warp": warp} if warp is not None else {}))
            if warp is not None and warp.last_grad_rts is not None:
                torch.autograd.backward(cams.get_rts(), warp.last_grad_rts)
            return loss
        for i in range(args.warmup):
            step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            step(args.warmup + i)
        torch.cuda.synchronize()
        res[f"warp_{leg}_ms_per_iteration"] = (time.perf_counter() - t0) / args.steps * 1e3
        timer = tm.KernelTimer()
        step(args.warmup + args.steps, timer)
        torch.cuda.synchronize()
        res[f"warp_{leg}_sections_ms"] = {k: round(v, 4) for k, v in timer.summary().items()}
        if warp is not None:
            with torch.no_grad():   # what the term saw at the last step: slots and neighbour rays
                fg = m.render_rays_fused(ro, rd, S, S, step0)
                q = torch.cat([fg["pred_depth"], fg["pred_diffuse"], fg["pred_specular"]], 1).contiguous()
                rv = fg["fore_valid"] | fg["bg_valid"]
                views, cost, valid = warp.select(ro, rd, q, rv)
                pr = warp.project(ro, rd, q, views, valid)
                res["rays_valid"] = int(rv.sum())
                res["slots_valid_after_selection"] = int(valid.sum())
                res["neighbour_rays_rendered"] = int(pr["valid"].sum())
                res["rays_with_10_candidates"] = int((valid.sum(1) == warp.K).sum())
                rts = cams.get_rts().detach()
                score = torch.rand(valid.shape, device=dev) * pr["valid"]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):   # the three warp kernels alone (no visibility render, no pose algebra)
                views, _, valid = warp.select(ro, rd, q, rv, rts)
                pr = warp.project(ro, rd, q, views, valid, rts)
                warp.loss_grad(ro, rd, q, rv, pr, score, 1.0, rts)
            torch.cuda.synchronize()
            res["warp_kernels_only_ms"] = (time.perf_counter() - t0) / args.steps * 1e3
        del m, opt
        torch.cuda.empty_cache()
    res.update({"rays": B, "cameras": args.cameras, "log2_T": args.log2_T, "samples": S, "image": [H, W],
                "device": torch.cuda.get_device_name(0)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
