"""Cost of the fused mesh's normals (csrc/tsdf.hip, scanerf_tsdf_vertex_normals) on the scene and cameras of
tools/bench_tsdf_fusion.py (3 x 3 tiles, a ring of `--cameras` views rendered at 1 / `--scale`), per lattice (`--cells` along the
box's longest side), on the mesh TSDFVolume.extract returns:

  * TSDFVolume.vertex_normals on the values / observed the extraction holds, `fused` (one launch) beside `composed` (the torch
    witness, one eager op per operation), compared BIT FOR BIT before anything is timed;
  * values + extraction (what the op follows) in the same visit, and extract(normals=True) beside extract();
  * vertices per second; the bytes of values / observed the op asks for per vertex (32 stencil points: 32 x 4 + 32 x 1, whatever
    the caches make of it) and the distinct stencil points over the whole mesh per vertex (what must come from memory at least
    once); the kernel's registers / LDS / scratch.

    python tools/bench_tsdf_normals.py [--cells 256,512] [--cameras 32] [--scale 4] [--repeats 9] [--composed-repeats 3]
                                       [--out profiles/tsdf_normals_bench.txt]

Host clock around work that ends in a device synchronise; every shape runs once before it is timed; medians.  Not measured: a real
capture's cameras, min_weight > 1, hardware counters."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def distinct_stencil_points(cells, n):
    """How many distinct lattice points the stencils of `cells` [V,3] touch (8 corners and 8 beyond them per axis, inside the lattice)."""
    c = cells.to(torch.int64)
    stride = ((n[1] + 1) * (n[2] + 1), n[2] + 1, 1)
    rows = []
    for d in range(8):
        o = (d >> 2, (d >> 1) & 1, d & 1)
        p = [c[:, k] + o[k] for k in range(3)]
        rows.append((p[0] * stride[0] + p[1] * stride[1]) + p[2])
        for a in range(3):
            q = list(p)
            q[a] = p[a] + (1 if o[a] else -1)
            ok = (q[a] >= 0) & (q[a] <= n[a])
            rows.append(((q[0] * stride[0] + q[1] * stride[1]) + q[2])[ok])
    return int(torch.unique(torch.cat(rows)).numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="256,512")
    ap.add_argument("--cameras", type=int, default=32)
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--log2-T", type=int, default=19)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--composed-repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    args = ap.parse_args()
    import scanerf_amd  # noqa
    from bench_mesh_visibility import kernel_resources
    from bench_scene_mesh import build_scene, clock
    from bench_tsdf_fusion import ring
    from scanerf_amd import _capi, fusion, meshing
    dev = "cuda:0"
    rnd = build_scene(dev, args.log2_T)
    corner, size = rnd.scene_box()
    center = [corner[k] + size[k] / 2 for k in range(3)]
    H, W = 1080, 1920
    ks, c2ws = ring(center, 1.1 * max(size), 0.5 * max(size), args.cameras, H, W, 1400.0)
    h, w = H // args.scale, W // args.scale
    k2 = fusion.scale_cameras(ks, args.scale).to(dev)
    c2ws = c2ws.to(dev)
    maps = []
    for K, c2w in zip(k2, c2ws):
        _, _, depth, transp = rnd.render(h, w, K, c2w)
        maps.append(fusion.mask_depth(depth[..., 0], transp[..., 0], 0.5))
    maps = torch.stack(maps).contiguous()
    res = {"device": torch.cuda.get_device_name(0), "tiles": int(rnd.feature_tables.shape[0]), "cameras": args.cameras, "frame": [h, w],
           "kernel": kernel_resources(_capi.LIB_PATH, "k_tsdf_vertex_normals"), "runs": {}}
    bits = lambda t: t.view(torch.int32)
    med = lambda f, k: statistics.median([clock(f)[0] for _ in range(1 + k)][1:])
    for cells in (int(s) for s in args.cells.split(",")):
        n = meshing.cells_per_axis(size, cells)
        spacing = fusion.lattice_spacing(size, n)
        vol = fusion.TSDFVolume(corner, spacing, n, fusion.default_trunc(spacing), dev)
        vol.integrate(maps, k2, c2ws)
        mesh = vol.extract()
        values, observed = vol.values(1)
        V = int(mesh.vertices.shape[0])
        fused = vol.vertex_normals(mesh, values=values, observed=observed)
        composed = vol.vertex_normals(mesh, values=values, observed=observed, route="composed")
        differ = int(((bits(fused[0]) != bits(composed[0])).any(1) | (bits(fused[1]) != bits(composed[1])).any(1)).sum())
        del composed
        op_ms = med(lambda: vol.vertex_normals(mesh, values=values, observed=observed), args.repeats)
        composed_ms = med(lambda: vol.vertex_normals(mesh, values=values, observed=observed, route="composed"), args.composed_repeats)
        extract_ms = med(lambda: vol.extract(), args.repeats)
        extract_normals_ms = med(lambda: vol.extract(normals=True), args.repeats)
        distinct = distinct_stencil_points(mesh.cells, n)
        res["runs"][str(cells)] = {
            "n": n, "points": vol.points, "V": V, "F": int(mesh.faces.shape[0]), "vertices_that_differ_fused_vs_composed": differ,
            "zero_normals": int((fused[0] == 0).all(1).sum()), "vertex_normals_ms": round(op_ms, 4), "composed_ms": round(composed_ms, 2),
            "composed_over_fused": round(composed_ms / op_ms, 1), "values_and_extraction_ms": round(extract_ms, 3),
            "values_extraction_and_normals_ms": round(extract_normals_ms, 3), "op_over_extraction": round(op_ms / extract_ms, 4),
            "vertices_per_s": round(V / op_ms * 1e3), "bytes_asked_per_vertex": {"values": 32 * 4, "observed": 32, "cells_lattice": 24, "outputs": 24},
            "distinct_stencil_points": distinct, "distinct_stencil_bytes_per_vertex": round(distinct * 5 / max(V, 1), 1),
            "asked_bytes_per_s": round(V * (32 * 5 + 48) / op_ms * 1e3)}
        del vol, mesh, values, observed, fused
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write(f"tools/bench_tsdf_normals.py --cells {args.cells} --cameras {args.cameras} --scale {args.scale} --repeats {args.repeats} "
                    f"--composed-repeats {args.composed_repeats}\n")
            f.write(line + "\n")


if __name__ == "__main__":
    main()
