"""Cost of the fused mesh extraction (csrc/isosurface.hip, meshing.extract_mesh) next to the density of its lattice alone:

  * `fused`    count pass (+ scan) and emit pass, timed separately, on a T = 2^19 f16 tile: lattices of 256^3 and 512^3 cells, at full
               occupancy and at tile_model.sphere_shell_occupancy;
  * `density`  render.sigma_normals_points over ALL lattice points of the same lattice (in slabs): what any composed route pays
               before it classifies anything -- a lower bound for it, and the baseline.

    python tools/bench_mesh_extract.py [--sizes 256,512] [--log2-T 19] [--repeats 5] [--out profiles/mesh_extract_bench.json]

Host clock around work that ends in a device synchronise; every shape is run once before it is timed; the shell comparison alternates
fused and density `repeats` times and reports each run, the ratio of the medians and the spread.  Writes one JSON document (rewritten
after every configuration, so a run that is cut short leaves what it measured)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--log2-T", type=int, default=19)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_extract_bench.json"))
    args = ap.parse_args()
    import scanerf_amd  # noqa
    from scanerf_amd import _capi, meshing, render
    from scanerf_amd import tile_model as tm
    dev = "cuda:0"
    lib = _capi.lib()
    m = tm.TileModel([-4.0, -4.0, -4.0], [8.0, 8.0, 8.0], dev, log2_T=args.log2_T, seed=24, table_dtype=torch.float16)
    with torch.no_grad():
        m.features.mul_(0.5 / float(m.features.std()))
    m.invalidate_gather_table()
    table, res, blob = m.gather_table().detach(), m.resolution, m.decoder.blob().detach().contiguous()
    wf = torch.ones(32, dtype=torch.float32, device=dev)
    log2dim = [int(v) for v in m.log2dim.tolist()]
    l2d = (ctypes.c_int32 * 3)(*log2dim)
    f3 = lambda t: (ctypes.c_float * 3)(*[float(v) for v in t.tolist()])
    sigma0, _, _ = render.sigma_normals_points(meshing.lattice_positions([32, 32, 32], dev), table, res, blob, wf)
    level = float(sigma0.median())
    occs = {"full": torch.ones_like(m.occupied_grid), "shell": tm.sphere_shell_occupancy(m, 2.5, 1.0)}
    out = {"device": torch.cuda.get_device_name(0), "log2_T": args.log2_T, "table": "f16", "level": level, "log2dim": log2dim, "runs": {}}

    def fused(n, occ):
        nbytes = lib.scanerf_isosurface_scratch_bytes(*n)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        head = (table.data_ptr(), _capi.F16, res.data_ptr(), blob.data_ptr(), wf.data_ptr(), table.shape[1], occ.data_ptr(), l2d, occ.numel(), *n, level)
        t_count, _ = clock(lambda: _capi.check(lib.scanerf_isosurface_count(*head, scratch.data_ptr(), nbytes, _capi.stream()), "count"))
        V, F = scratch[:16].view(torch.int64).tolist()
        bufs = [torch.empty((V, 3), dtype=torch.float32, device=dev), torch.empty((F, 3), dtype=torch.int32, device=dev),
                torch.empty((V, 3), dtype=torch.int32, device=dev)]
        t_emit, _ = clock(lambda: _capi.check(lib.scanerf_isosurface_emit(*head, f3(m.occ_corner), f3(m.occ_size), scratch.data_ptr(), nbytes,
                                                                          bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), None, V, F,
                                                                          _capi.stream()), "emit"))
        return {"count_ms": t_count, "emit_ms": t_emit, "total_ms": t_count + t_emit, "V": V, "F": F, "scratch_bytes": nbytes}

    def density(n):
        def run():
            h = [float(torch.tensor(2.0) / torch.tensor(float(v))) for v in n]
            ay = torch.arange(n[1] + 1, device=dev, dtype=torch.float32) * h[1] - 1.0
            az = torch.arange(n[2] + 1, device=dev, dtype=torch.float32) * h[2] - 1.0
            slab = max(1, (1 << 24) // ((n[1] + 1) * (n[2] + 1)))
            for i0 in range(0, n[0] + 1, slab):
                ax = torch.arange(i0, min(i0 + slab, n[0] + 1), device=dev, dtype=torch.float32) * h[0] - 1.0
                x = torch.stack(torch.meshgrid(ax, ay, az, indexing="ij"), -1).reshape(-1, 3).contiguous()
                render.sigma_normals_points(x, table, res, blob, wf)
        return clock(run)[0]

    def live_bricks(n, occ):
        live = meshing.live_points(n, occ).float()[None, None]
        pad = [0, (-n[2]) % 8, 0, (-n[1]) % 8, 0, (-n[0]) % 8]
        b = torch.nn.functional.max_pool3d(torch.nn.functional.pad(live, pad), kernel_size=9, stride=8)
        return float(b.mean()), float(live.mean())

    for size in (int(s) for s in args.sizes.split(",")):
        n = [size, size, size]
        row = {"points": (size + 1) ** 3, "cells": size ** 3}
        for name, occ in occs.items():
            fused(n, occ)                                  # warm
            r = fused(n, occ)
            r["live_brick_fraction"], r["live_point_fraction"] = live_bricks(n, occ)
            row[name] = r
            out["runs"][str(size)] = row
            json.dump(out, open(args.out, "w"), indent=1)
        density(n)                                         # warm
        pairs = []
        for _ in range(args.repeats):                      # alternating: fused on the shell, then the density of the whole lattice
            pairs.append({"fused_shell_ms": fused(n, occs["shell"])["total_ms"], "density_all_points_ms": density(n)})
        fm, dm = (statistics.median(p[k] for p in pairs) for k in ("fused_shell_ms", "density_all_points_ms"))
        row["alternating"] = pairs
        row["fused_shell_median_ms"], row["density_median_ms"] = fm, dm
        row["density_over_fused_shell"] = dm / fm
        row["spread"] = {k: (max(p[k] for p in pairs) - min(p[k] for p in pairs)) / statistics.median(p[k] for p in pairs)
                         for k in ("fused_shell_ms", "density_all_points_ms")}
        out["runs"][str(size)] = row
        json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
