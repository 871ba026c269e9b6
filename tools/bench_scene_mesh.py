"""Cost of the scene mesh (csrc/isosurface.hip's scene source, meshing.extract_scene_mesh) next to the composed route:

  * `fused`     scanerf_isosurface_count_tiles (+ scan) and scanerf_isosurface_emit_tiles, timed separately, on a 3 x 3 grid of
                T = 2^19 f16 tiles (4 x 4 x 4 on a pitch of 3 in x and z, as tests/render_scenes.py lays scenes out) with sphere-shell
                occupancies, on two lattices over the bounding box of the tiles;
  * `composed`  the same field from the ops the package had before: per tile, on the device, positions / membership / weights /
                occupancy of the lattice points the tile holds (torch), render.sigma_normals_points at the contributing points,
                the blend into a lattice of sums and a lattice of weights, then meshing.surface_nets on the stored lattice.  The
                baseline, in time and in the bytes it holds (torch.cuda.max_memory_allocated above the resident tiles).

    python tools/bench_scene_mesh.py [--cells 256,512] [--log2-T 19] [--repeats 5] [--out profiles/scene_mesh_bench.json]

Host clock around work that ends in a device synchronise; every shape is run once before it is timed; fused and composed alternate
`repeats` times and every run is reported, with the medians, their ratio and the spread.  The composed route's device division and
torch's elementwise kernels are not pinned to the definition: its V and F are reported beside the fused route's, not compared bit for
bit (tests/test_gpu_scene_mesh.py does that against the host witness).  Writes one JSON document, rewritten after every lattice."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def build_scene(dev, log2_T, grid=(3, 3)):
    """-> renderer.TileSetRenderer of grid[0] x grid[1] tiles with sphere-shell occupancies (radius 1.4, thickness 0.7 around each
    tile's centre: neighbouring shells cross in the margins) and tables scaled to a standard deviation of 0.5."""
    from scanerf_amd import renderer
    from scanerf_amd import tile_model as tm
    tiles = []
    for ix in range(grid[0]):
        for iz in range(grid[1]):
            m = tm.TileModel([3.0 * ix, -2.0, 3.0 * iz], [4.0, 4.0, 4.0], dev, log2_T=log2_T, seed=40 + ix * grid[1] + iz, table_dtype=torch.float16)
            with torch.no_grad():
                m.features.mul_(0.5 / float(m.features.std()))
            m.invalidate_gather_table()
            m.set_occupancy(tm.sphere_shell_occupancy(m, 1.4, 0.7))
            c = lambda t: t.detach().cpu().numpy()
            tiles.append({"features": c(m.gather_table()), "occupied_grid": c(m.occupied_grid), "block_corner": c(m.min_bbox),
                          "block_size": c(m.bbox_size), "grid_log2dim": c(m.log2dim), "resolution": c(m.resolution), "blob": c(m.decoder.blob())})
            del m
    torch.cuda.empty_cache()
    return renderer.TileSetRenderer(dev, tiles)


def composed(rnd, corner, size, n, level):
    """The composed route on the device -> (Mesh, evaluated points)."""
    from scanerf_amd import meshing, render
    dev, f32 = rnd.device, torch.float32
    step = [float(np.float32(size[k]) / np.float32(n[k])) for k in range(3)]
    wp = [corner[k] + torch.arange(n[k] + 1, device=dev, dtype=f32) * step[k] for k in range(3)]
    num = torch.zeros([m + 1 for m in n], dtype=f32, device=dev)
    W = torch.zeros_like(num)
    ones = torch.ones(32, dtype=f32, device=dev)
    cn, sz, l2d, starts = rnd.block_corner.cpu(), rnd.block_size.cpu(), rnd.grid_log2dim.cpu().tolist(), rnd.grid_starts.cpu().tolist()
    evaluated = 0
    for b in range(cn.shape[0]):
        pt, sl = [], []
        for k in range(3):
            p = (wp[k] - float(cn[b, k])) / float(sz[b, k])
            idx = torch.nonzero((p >= 0) & (p <= 1)).flatten()
            if idx.numel() == 0:
                break
            sl.append(slice(int(idx[0]), int(idx[-1]) + 1))
            pt.append(p[sl[-1]])
        if len(sl) < 3:
            continue
        dis = [(0.5 - (pt[k] - 0.5).abs()) * float(sz[b, k]) for k in range(3)]
        dx, dz = dis[0][:, None], dis[2][None, :]
        w2 = torch.where((dx != 0) & (dz != 0), dx * dz, torch.where(dx != 0, dx, torch.where(dz != 0, dz, torch.zeros_like(dz))))
        loc = [(pt[k] * float(2 ** l2d[b][k])).to(torch.int64).clamp_(0, 2 ** l2d[b][k] - 1) for k in range(3)]
        off = (loc[0][:, None, None] << (l2d[b][1] + l2d[b][2])) | (loc[1][None, :, None] << l2d[b][2]) | loc[2][None, None, :]
        run = rnd.occupied_grid[starts[b] + off]
        W[sl[0], sl[1], sl[2]] += w2[:, None, :]
        i = torch.nonzero(run)
        if i.shape[0]:
            x = torch.stack([2.0 * pt[k][i[:, k]] - 1.0 for k in range(3)], 1).contiguous()
            sigma, _, _ = render.sigma_normals_points(x, rnd.feature_tables[b], rnd.resolution[b], rnd.params[b], ones)
            evaluated += int(x.shape[0])
            sub = num[sl[0], sl[1], sl[2]]
            sub[run] += w2[i[:, 0], i[:, 2]] * sigma
    values = num * torch.where(W > 0, 1.0 / W, torch.ones_like(W))
    del num, W
    return meshing.surface_nets(values, level, corner, step), evaluated


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="256,512", help="lattice cells along the scene box's longest side, one lattice each")
    ap.add_argument("--log2-T", type=int, default=19)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_mesh_bench.json"))
    args = ap.parse_args()
    import scanerf_amd  # noqa
    from scanerf_amd import _capi, meshing, render
    dev = "cuda:0"
    lib = _capi.lib()
    rnd = build_scene(dev, args.log2_T)
    corner, size = rnd.scene_box()
    nb, T = int(rnd.feature_tables.shape[0]), int(rnd.feature_tables.shape[2])
    x0 = meshing.lattice_positions([32, 32, 32], dev)
    sigma0, _, _ = render.sigma_normals_points(x0, rnd.feature_tables[0], rnd.resolution[0], rnd.params[0], torch.ones(32, device=dev))
    level = float(sigma0.median())
    f3 = lambda v: (ctypes.c_float * 3)(*[float(x) for x in v])
    out = {"device": torch.cuda.get_device_name(0), "tiles": nb, "log2_T": args.log2_T, "table": "f16", "level": level,
           "box_corner": corner, "box_size": size, "occupancy": "sphere shell, radius 1.4, thickness 0.7, per tile",
           "occupied_fraction": float(rnd.occupied_grid.float().mean()), "runs": {}}

    def fused(n):
        nbytes = lib.scanerf_isosurface_scratch_bytes(*n)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        head = (rnd.feature_tables.data_ptr(), rnd.params.data_ptr(), rnd.resolution.data_ptr(), rnd.occupied_grid.data_ptr(),
                rnd.grid_starts.data_ptr(), rnd.grid_log2dim.data_ptr(), rnd.block_corner.data_ptr(), rnd.block_size.data_ptr(), T, nb,
                f3(corner), f3(size), *n, level)
        t_count, _ = clock(lambda: _capi.check(lib.scanerf_isosurface_count_tiles(*head, scratch.data_ptr(), nbytes, _capi.stream()), "count"))
        V, F = scratch[:16].view(torch.int64).tolist()
        bufs = [torch.empty((V, 3), dtype=torch.float32, device=dev), torch.empty((F, 3), dtype=torch.int32, device=dev),
                torch.empty((V, 3), dtype=torch.int32, device=dev), torch.empty((V, 3), dtype=torch.float32, device=dev)]
        t_emit, _ = clock(lambda: _capi.check(lib.scanerf_isosurface_emit_tiles(*head, scratch.data_ptr(), nbytes, bufs[0].data_ptr(),
                                                                                bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(), V, F,
                                                                                _capi.stream()), "emit"))
        return {"count_ms": t_count, "emit_ms": t_emit, "total_ms": t_count + t_emit, "V": V, "F": F, "scratch_bytes": nbytes,
                "output_bytes": sum(b.numel() * b.element_size() for b in bufs)}

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        ms, r = clock(fn)
        return ms, torch.cuda.max_memory_allocated() - before, r

    for cells in (int(s) for s in args.cells.split(",")):
        n = meshing.cells_per_axis(size, cells)
        row = {"n": n, "points": int(np.prod([m + 1 for m in n])), "cells": int(np.prod(n))}
        fused(n)                                            # warm
        composed(rnd, corner, size, n, level)               # warm
        f = fused(n)
        _, f["peak_bytes"], _ = peak(lambda: rnd.extract_mesh(level, cells))
        ms, pk, (mesh, evaluated) = peak(lambda: composed(rnd, corner, size, n, level))
        row["fused"] = f
        row["composed"] = {"total_ms": ms, "peak_bytes": pk, "V": int(mesh.vertices.shape[0]), "F": int(mesh.faces.shape[0]),
                           "evaluated_points": evaluated,
                           "output_bytes": sum(t.numel() * t.element_size() for t in (mesh.vertices, mesh.faces, mesh.cells, mesh.lattice))}
        del mesh
        pairs = []
        for _ in range(args.repeats):                       # alternating
            r = fused(n)
            pairs.append({"fused_count_ms": r["count_ms"], "fused_emit_ms": r["emit_ms"], "fused_ms": r["total_ms"],
                          "composed_ms": clock(lambda: composed(rnd, corner, size, n, level))[0]})
        fm, cm = (statistics.median(p[k] for p in pairs) for k in ("fused_ms", "composed_ms"))
        row["alternating"] = pairs
        row["fused_median_ms"], row["composed_median_ms"], row["composed_over_fused"] = fm, cm, cm / fm
        row["spread"] = {k: (max(p[k] for p in pairs) - min(p[k] for p in pairs)) / statistics.median(p[k] for p in pairs)
                         for k in ("fused_ms", "composed_ms")}
        out["runs"][str(cells)] = row
        json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
