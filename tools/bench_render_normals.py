"""Cost of the multi-tile renderer's normal map (csrc/render_normals_tiles.hip, renderer.TileSetRenderer normals=True) on the frame
of bench.py's render leg: 1920 x 1080, 4 tiles (f16 tables T = 2^19, shell occupancy) + blended backgrounds, 128 + 128 samples.

  * `frame`   rend.render(...) with normals off and on, --repeats times --steps frames each (host clock around work that ends in a
              device synchronise), every repeat and its spread reported;
  * `ops`     pts_normals alone against pts_inference on the SAME inputs: the arguments of every tracing pass of one normals=True
              frame are captured (rays, depths, slot lists, in the renderer's layout) and both ops are timed on them;
  * `counts`  the counted launch of pts_normals on those inputs: 64-sample groups that ran a tile, stagings of a tile's operands in
              LDS, passes of the per-tile loop and the lanes that held a sample in them, and the launch's waves -> restagings per wave
              and per group, lane utilisation.

    python tools/bench_render_normals.py [--steps 5] [--warmup 2] [--repeats 5] [--pitch 8.0] [--legs frame,ops,counts]

--pitch: distance between the tiles' corners along x (8 = bench.py's frame: the tiles touch; smaller: they overlap and samples list
two tiles).  One JSON line -> profiles/render_normals_bench.json.  For a kernel trace run one leg on its own under
`rocprofv3 --kernel-trace --stats -- python tools/bench_render_normals.py --legs ops`."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_renderer(dev, ntile, log2_T, pitch):
    """bench.py time_render's scene (tile t spans [-4 ntile + pitch t, +8] x [-4,4] x [-4,4])"""
    from scanerf_amd import renderer as R
    from scanerf_amd import tile_model as tm
    tiles = []
    with tempfile.TemporaryDirectory() as tmp:
        for t in range(ntile):
            m = tm.TileModel([-4.0 * ntile + pitch * t, -4, -4], [8, 8, 8], dev, log2_T=log2_T, seed=t, sampler_log2dim=7)
            m.set_occupancy(tm.sphere_shell_occupancy(m, 3.0, 0.5))
            with torch.no_grad():
                m.features.mul_(300.0)
            R.export_tile(os.path.join(tmp, f"tile{t}"), m)
            tiles.append(R.load_tile(os.path.join(tmp, f"tile{t}")))
            del m
    return R.TileSetRenderer(dev, tiles)


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def spread(v):
    return {"ms": [round(x, 3) for x in v], "min": round(min(v), 3), "median": round(sorted(v)[len(v) // 2], 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--log2-T", type=int, default=19)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--tiles", type=int, default=4)
    ap.add_argument("--pitch", type=float, default=8.0)
    ap.add_argument("--legs", default="frame,ops,counts")
    args = ap.parse_args()
    import scanerf_amd  # noqa
    from scanerf_amd import hashgrid as HG
    from scanerf_amd import renderer as R
    dev, legs, S = "cuda:0", args.legs.split(","), args.samples
    H, W = 1080, 1920
    rend = build_renderer(dev, args.tiles, args.log2_T, args.pitch)
    K = [1600.0, 0, W / 2, 0, 1600.0, H / 2, 0, 0, 1]
    c2w = torch.tensor([[1.0, 0, 0, 0.0], [0, 1, 0, 0.5], [0, 0, 1, -14.0]])
    frame = lambda nm: rend.render(H, W, K, c2w, num_sample=S, num_bg_sample=S, normals=nm)
    out = {"frame": f"{W}x{H}, {args.tiles} tiles at pitch {args.pitch} (f16 tables T=2^{args.log2_T}, shell occupancy) + blended backgrounds, "
                    f"{S} + {S} samples", "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats}
    if "frame" in legs:
        off, on = [], []
        for _ in range(args.repeats):   # interleaved: drift lands on both
            off.append(timed(lambda: frame(False), args.warmup, args.steps))
            on.append(timed(lambda: frame(True), args.warmup, args.steps))
        out["frame_normals_off_ms"], out["frame_normals_on_ms"] = spread(off), spread(on)
        nm = frame(True)[4]
        out["normal_map"] = {"covered_fraction": float((nm.norm(dim=-1) > 0.5).float().mean()), "max_norm": float(nm.norm(dim=-1).max())}
    if "ops" in legs or "counts" in legs:
        # the arguments of every tracing pass of one frame, as the renderer hands them to pts_normals
        passes, real = [], R.pts_normals

        def capture(*a, **k):
            passes.append(([t.clone() for t in a[:5]], k.get("sample_major", 0)))
            return real(*a, **k)
        R.pts_normals = capture
        try:
            frame(True)
        finally:
            R.pts_normals = real
        scene = (rend.feature_tables, rend.resolution, rend.occupied_grid, rend.grid_starts, rend.grid_log2dim, rend.block_corner,
                 rend.block_size)
        rows = []
        for (ro, rd, z, dd, bi), sm in passes:
            n_rays = ro.shape[0]
            listed = bi.reshape(-1, 4)
            row = {"rays": n_rays, "samples": n_rays * S, "layout": sm, "listed_fraction": float((listed[:, 0] != -1).float().mean()),
                   "two_or_more_fraction": float((listed[:, 1] != -1).float().mean())}
            pd, ps = torch.empty(*z.shape, 3, device=dev), torch.empty(*z.shape, 3, device=dev)
            pa, pn = torch.empty(*z.shape, 1, device=dev), torch.empty(*z.shape, 3, device=dev)
            inference = lambda: HG.pts_inference(ro, rd, z, dd, bi, scene[0], rend.packed, *scene[1:], pd, ps, pa, sample_major=sm)
            normals = lambda c=None: HG.pts_normals(ro, rd, z, dd, bi, scene[0], rend.params, *scene[1:], pn, sample_major=sm, counts=c)
            if "ops" in legs:
                a, b = [], []
                for _ in range(args.repeats):
                    a.append(timed(inference, args.warmup, args.steps))
                    b.append(timed(normals, args.warmup, args.steps))
                row["pts_inference_ms"], row["pts_normals_ms"] = spread(a), spread(b)
                row["normals_over_inference"] = round(row["pts_normals_ms"]["median"] / row["pts_inference_ms"]["median"], 3)
            if "counts" in legs:
                c = torch.zeros(4, dtype=torch.int32, device=dev)
                normals(c)
                groups, stagings, loops, lanes = (int(v) for v in c.cpu())
                waves = min((n_rays * S + 63) // 64, 256 * 8)   # kTnMaxBlocks of one wave each
                row.update(groups_total=(n_rays * S + 63) // 64, groups_run=groups, stagings=stagings, waves=waves,
                           stagings_per_wave=round(stagings / waves, 2), stagings_per_run_group=round(stagings / max(groups, 1), 4),
                           tile_loop_passes=loops, lanes_with_a_sample=lanes, lane_utilisation=round(lanes / max(64 * loops, 1), 4))
            rows.append(row)
        out["passes"] = rows
    print(json.dumps(out))


if __name__ == "__main__":
    main()
