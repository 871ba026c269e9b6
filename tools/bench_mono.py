"""Cost of the monocular prior terms (scanerf_amd.mono, csrc/mono.hip) on the reference's shipped iteration: T = 2^24, 16 384 rays,
foreground + T_left * background (128 + 128 samples), pose refinement (train_step_fgbg(pose_grads=True), bench.py's
reference_default leg) -- timed with the terms off and on (weights 0.01 / 0.001, as config/default.yaml ships them).

    python tools/bench_mono.py [--steps 20] [--warmup 3] [--cameras 64]

The batch is laid out as tile.py draws it: rays / cameras rays per view, 2x2 patches, the same pixel set in every view
(trainer.sample_patch_ray_idx, cameras.pixel_locs).  The monocular maps are procedural (a depth ramp, normals facing the camera).
Also reports the mono kernels alone (one scanerf_mono_loss_grad call).  One JSON line.  For the per-kernel split run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_mono.py`."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cameras", type=int, default=64)
    ap.add_argument("--rays", type=int, default=16384)
    ap.add_argument("--log2-T", type=int, default=24)
    ap.add_argument("--samples", type=int, default=128)
    args = ap.parse_args()
    import scanerf_amd  # noqa
    from scanerf_amd import cameras as CM
    from scanerf_amd import tile_model as tm
    from scanerf_amd.mono import MonoLoss
    from scanerf_amd.trainer import sample_patch_ray_idx
    from bench_warp import camera_block
    dev = "cuda:0"
    H, W, S, N = 300, 400, args.samples, args.cameras
    cams = camera_block(N, H, W, 200.0, dev)
    g = torch.Generator(device=dev).manual_seed(25)
    idx = sample_patch_ray_idx(args.rays, N, H, W, dev, generator=g)
    locs = CM.pixel_locs(N, idx, W, dev)
    B = locs.shape[0]
    tg = torch.rand(B, 3, device=dev, generator=g)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    md = (3.0 + 0.002 * xx + 0.001 * yy)[None].expand(N, H, W).contiguous().float()
    mn = torch.nn.functional.normalize(torch.stack([0.05 * torch.ones_like(md), 0.02 * torch.ones_like(md), -torch.ones_like(md)], -1), dim=-1)
    ks = cams.ks.detach().float().cpu()
    step0 = 20000
    res = {}
    ro, rd = (x.detach().contiguous() for x in cams.get_rays(locs))
    for leg in ("off", "on"):
        m = tm.TileModel([-4.0, -4, -4], [8, 8, 8], dev, log2_T=args.log2_T, seed=24, sampler_log2dim=4)
        opt = torch.optim.Adam(m.decoder.parameters(), lr=1e-3, betas=(0.9, 0.99), eps=1e-15)
        mono = MonoLoss(ks, md, mn, end_step=40000) if leg == "on" else None
        kw = {} if mono is None else {"mono": mono, "locs": locs}

        def step(i, timer=None):
            return tm.train_step_fgbg(m, opt, ro, rd, tg, S, S, step0 + i, pose_grads=True, timer=timer, **kw)
        for i in range(args.warmup):
            step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            step(args.warmup + i)
        torch.cuda.synchronize()
        res[f"mono_{leg}_ms_per_iteration"] = (time.perf_counter() - t0) / args.steps * 1e3
        timer = tm.KernelTimer()
        step(args.warmup + args.steps, timer)
        torch.cuda.synchronize()
        res[f"mono_{leg}_sections_ms"] = {k: round(v, 4) for k, v in timer.summary().items()}
        if mono is not None:
            res["last_depth_loss"] = float(mono.last_depth_loss)
            res["last_smooth_loss"] = float(mono.last_smooth_loss)
            with torch.no_grad():
                fg = m.render_rays_fused(ro, rd, S, S, step0)
                depth = fg["pred_depth"][:, 0].contiguous()
                rv = (fg["fore_valid"] | fg["bg_valid"]).contiguous()
            res["rays_valid"] = int(rv.sum())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):   # the mono kernels alone (one scanerf_mono_loss_grad call)
                mono.loss_grad(locs, depth, rv, 0.01, 0.001)
            torch.cuda.synchronize()
            res["mono_kernels_only_ms"] = (time.perf_counter() - t0) / args.steps * 1e3
        del m, opt
        torch.cuda.empty_cache()
    res["mono_overhead_ms"] = res["mono_on_ms_per_iteration"] - res["mono_off_ms_per_iteration"]
    res.update({"rays": B, "cameras": N, "log2_T": args.log2_T, "samples": S, "image": [H, W],
                "device": torch.cuda.get_device_name(0)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
