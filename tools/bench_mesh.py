"""Cost of the mesh tracer (scanerf_amd.fastmesh, csrc/mesh.hip): structure build, first_hit / first_enter rates, the kernel
alternatives side by side in one run, and the "BS" background mode beside "IZ" on the reference's shipped iteration shape.

    python tools/bench_mesh.py [--repeat 20] [--warmup 3] [--large-n 1000] [--no-step]

Meshes: the tests' terrain fixture (48 x 48 height field + 12 boxes: 4 752 faces) and a procedural height field of
2 * large_n^2 faces (default 2 000 000) made on the device.  Ray sets: one 1920 x 1080 camera frame in image order, the same
frame re-tiled into 8 x 8 pixel blocks (one block per wavefront), and a 16 384-ray random training batch.  Every figure is the
median of `repeat` launches after `warmup`, timed with HIP events.  Variants of first_hit: pre-gathered triangles (36 B per
face-list entry) or indexed faces; bitmask + rank read from global memory or staged into the LDS.  One JSON line.  For the
per-kernel split: `rocprofv3 --kernel-trace --stats -- python tools/bench_mesh.py --no-step`."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def event_ms(fn, repeat, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def height_field(n, dev):
    """2 n^2 faces over [-10,10]^2 with 40 box-like towers: a scene-scale mesh made in memory."""
    xs = torch.linspace(-10, 10, n + 1, device=dev)
    X, Y = torch.meshgrid(xs, xs, indexing="ij")
    Z = 0.8 * torch.sin(0.6 * X) * torch.cos(0.5 * Y) + 0.05 * torch.sin(7.0 * X + 3.0 * Y)
    g = torch.Generator(device="cpu").manual_seed(3)
    for _ in range(40):
        cx, cy = (torch.rand(2, generator=g) * 16 - 8).tolist()
        w, h = (torch.rand(2, generator=g) * 1.5 + 0.3).tolist()
        Z = torch.where(((X - cx).abs() < w) & ((Y - cy).abs() < w), Z + h, Z)
    V = torch.stack([X, Y, Z], -1).reshape(-1, 3).float()
    i, j = torch.meshgrid(torch.arange(n, device=dev), torch.arange(n, device=dev), indexing="ij")
    q = lambda a, b: (a * (n + 1) + b).reshape(-1)
    F = torch.cat([torch.stack([q(i, j), q(i + 1, j), q(i + 1, j + 1)], -1), torch.stack([q(i, j), q(i + 1, j + 1), q(i, j + 1)], -1)])
    return V.contiguous(), F.int().contiguous()


def build_ms(V, F, dev, repeat=3, **kw):
    from scanerf_amd.fastmesh import FastMesh
    times = []
    for _ in range(repeat + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fm = FastMesh.from_arrays(V, F, dev, **kw)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return fm, float(np.median(times[1:]))


def block_order(H, W, b=8):
    """Pixel indices of an H x W frame, 8 x 8 blocks one after another (64 consecutive rays = one block = one wavefront)."""
    idx = torch.arange(H * W).reshape(H // b, b, W // b, b).permute(0, 2, 1, 3).reshape(-1)
    return idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--large-n", type=int, default=1000)
    ap.add_argument("--no-step", action="store_true", help="skip the BS / IZ training iterations")
    ap.add_argument("--rays", type=int, default=16384)
    ap.add_argument("--log2-T", type=int, default=24)
    ap.add_argument("--samples", type=int, default=128)
    args = ap.parse_args()
    import fastmesh_reference as FR
    import scanerf_amd  # noqa
    from scanerf_amd import tile_model as tm
    from scanerf_amd.fastmesh import FastMesh
    dev = "cuda:0"
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "repeat": args.repeat}
    H, W = 1080, 1920
    c2w, K = FR.look_at([13.0, -9.0, 5.0], [0.0, 0.0, 0.0], H, W, 1400.0)
    o, d = (T(x) for x in FR.camera_rays(c2w, K, H, W))
    perm = block_order(H, W).to(dev)
    g = torch.Generator(device="cpu").manual_seed(1)
    ro = torch.stack([torch.rand(args.rays, generator=g) * 18 - 9, torch.rand(args.rays, generator=g) * 18 - 9,
                      torch.rand(args.rays, generator=g) * 4.5 + 1.5], -1).to(dev)
    rd = torch.randn(args.rays, 3, generator=g)
    rd[:, 2] -= 0.6
    rd = torch.nn.functional.normalize(rd, dim=-1).to(dev)
    sets = {"frame_image_order": (o, d), "frame_8x8_blocks": (o[perm].contiguous(), d[perm].contiguous()), "batch_random": (ro, rd)}

    Vf, Ff, _ = FR.terrain_fixture()
    meshes = {"fixture": (T(Vf), T(Ff))}
    if args.large_n > 0:
        meshes["large"] = height_field(args.large_n, dev)
    for mname, (V, F) in meshes.items():
        fm, ms = build_ms(V, F, dev)
        _, ms_idx = build_ms(V, F, dev, pregather=False)
        r = {"faces": int(F.shape[0]), "vertices": int(V.shape[0]), "occupied_cells": fm.num_cells, "list_entries": int(fm.cell_faces.shape[0]),
             "build_ms": round(ms, 3), "build_indexed_only_ms": round(ms_idx, 3),
             "bytes_pregathered": int(fm.tris.numel() * 4) if fm.tris is not None else 0,
             "bytes_indexed": int(fm.cell_faces.numel() * 4 + fm.faces.numel() * 4 + fm.vertices.numel() * 4)}
        tris = fm.tris
        for sname, (so, sd) in sets.items():
            n = so.shape[0]
            out = torch.empty(n, device=dev)
            for pre in ((True, False) if tris is not None else (False,)):
                for lds in (False, True):
                    fm.tris, fm.lds = (tris if pre else None), lds
                    ms = event_ms(lambda: fm.first_hit(so, sd, out=out), args.repeat, args.warmup)
                    r[f"first_hit.{sname}.{'pregathered' if pre else 'indexed'}.{'lds' if lds else 'global'}"] = {
                        "ms": round(ms, 4), "Mrays_per_s": round(n / ms / 1e3, 1)}
            fm.tris = tris
            for lds in (False, True):
                fm.lds = lds
                ms = event_ms(lambda: fm.first_enter(so, sd, out=out), args.repeat, args.warmup)
                r[f"first_enter.{sname}.{'lds' if lds else 'global'}"] = {"ms": round(ms, 4), "Mrays_per_s": round(n / ms / 1e3, 1)}
            fm.lds = False
            r[f"hit_share.{sname}"] = round(float((fm.first_hit(so, sd) > 0).float().mean()), 3)
        fm.set(torch.tensor([0.0, 0.0, 0.5]), torch.tensor([6.0, 6.0, 3.0]))
        r["render_mask.frame_ms"] = round(event_ms(lambda: fm.render_mask(o, d), args.repeat, args.warmup), 4)
        res[mname] = r
        del fm, tris
        torch.cuda.empty_cache()

    if not args.no_step:   # the reference's shipped iteration shape, fg + bg: "IZ" beside "BS" (two more traces per step)
        Vs, Fs = FR.shell_fixture()
        fm = FastMesh.from_arrays(Vs, Fs, dev)
        B, S = args.rays, args.samples
        so = (torch.rand(B, 3, generator=g) * 7.0 - 3.5).to(dev)
        sd = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1).to(dev)
        tg = torch.rand(B, 3, generator=g).to(dev)
        for mode in ("IZ", "BS", "IZ", "BS"):   # each mode twice, interleaved: the second pair shows the run-to-run spread
            m = tm.TileModel([-4.0, -4, -4], [8, 8, 8], dev, log2_T=args.log2_T, seed=24, sampler_log2dim=4)
            fm.set(m._center_dev, m._half_dev)
            opt = torch.optim.Adam(m.decoder.parameters(), lr=1e-3, betas=(0.9, 0.99), eps=1e-15)
            kw = {"bg_mode": "BS", "fmesh": fm} if mode == "BS" else {}
            i = [0]

            def step():
                tm.train_step_fgbg(m, opt, so, sd, tg, S, S, 20000 + i[0], **kw)
                i[0] += 1
            res.setdefault(f"step_{mode}_ms", []).append(round(event_ms(step, args.repeat, args.warmup), 4))
            if mode == "BS":
                res["bs_sampling_only_ms"] = round(event_ms(lambda: tm.mesh_background_samples(fm, so, sd, S, m.bbox_size.tolist()),
                                                            args.repeat, args.warmup), 4)
                res["iz_sampling_only_ms"] = round(event_ms(lambda: m.inverse_z_sampling(so, sd, S), args.repeat, args.warmup), 4)
            del m, opt
            torch.cuda.empty_cache()
        res["step"] = {"rays": B, "samples": S, "log2_T": args.log2_T}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
