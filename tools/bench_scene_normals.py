"""Cost of the blended density's gradient at a scene mesh's vertices (csrc/scene_normals.hip, meshing.scene_sigma_normals_points;
DESIGN.md 4.16) next to the composed route and to the extraction itself:

  * `fused`     scanerf_scene_sigma_normals_points at the vertices of tools/bench_scene_mesh.py's scene (3 x 3 tiles, T = 2^19 f16,
                sphere-shell occupancies) on its two lattices, in the mesh's brick order and in one random permutation of it (what the
                brick order is worth to the staging);
  * `composed`  the same quantity from the ops the package had before, all on the device: per tile, torch membership / weights /
                weight gradients / occupancy of all vertices, render.sigma_normals_points(want_grad=True) at the contributing ones
                (an index array per tile), the sums and the quotient rule in torch;
  * `extract`   the extraction's own count + emit time on the same lattice.

    python tools/bench_scene_normals.py [--cells 256,512] [--log2-T 19] [--repeats 5] [--out profiles/scene_normals_bench.json]

Host clock around work that ends in a device synchronise; every shape is run once before it is timed; the routes alternate `repeats`
times and every run is reported, with the medians, their ratios and the spread.  torch's elementwise kernels are not pinned to the
definition: the composed route's result is compared with the fused one by its largest difference over the conditioning-free scale
|g|, not bit for bit (tests/test_gpu_scene_normals.py does that against the host witness).  One JSON document, rewritten per lattice."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def composed(rnd, p):
    """The composed route on the device -> (sigma, grad, evaluated points)."""
    from scanerf_amd import render
    dev, f32 = rnd.device, torch.float32
    N = p.shape[0]
    W, num = torch.zeros(N, dtype=f32, device=dev), torch.zeros(N, dtype=f32, device=dev)
    A, B, C = (torch.zeros((N, 3), dtype=f32, device=dev) for _ in range(3))
    ones = torch.ones(32, dtype=f32, device=dev)
    hit = torch.zeros(N, dtype=torch.bool, device=dev)
    l2d, starts, sizes = rnd.grid_log2dim.cpu().tolist(), rnd.grid_starts.cpu().tolist(), rnd.block_size.cpu().tolist()
    evaluated = 0
    for b in range(rnd.block_corner.shape[0]):
        pt = (p - rnd.block_corner[b]) / rnd.block_size[b]
        listed = ((pt >= 0) & (pt <= 1)).all(1)
        dis = (0.5 - (pt - 0.5).abs()) * rnd.block_size[b]
        dx, dz = dis[:, 0], dis[:, 2]
        side = torch.sign(0.5 - pt)
        both, ox, oz = (dx != 0) & (dz != 0), (dx != 0) & (dz == 0), (dx == 0) & (dz != 0)
        zero = torch.zeros_like(dx)
        w = torch.where(both, dx * dz, torch.where(ox, dx, torch.where(oz, dz, zero)))
        gw = torch.stack([torch.where(both, side[:, 0] * dz, torch.where(ox, side[:, 0], zero)), zero,
                          torch.where(both, side[:, 2] * dx, torch.where(oz, side[:, 2], zero))], 1)
        W += torch.where(listed, w, zero)
        C += torch.where(listed[:, None], gw, torch.zeros_like(gw))
        r = torch.tensor([2 ** k for k in l2d[b]], device=dev)
        loc = torch.minimum((pt * r).to(torch.int64).clamp_(min=0), r - 1)
        off = (loc[:, 0] << (l2d[b][1] + l2d[b][2])) | (loc[:, 1] << l2d[b][2]) | loc[:, 2]
        run = listed & rnd.occupied_grid[starts[b] + off]
        i = torch.nonzero(run).flatten()
        if i.numel() == 0:
            continue
        x = (2.0 * pt[i] - 1.0).contiguous()
        sigma, grad, _ = render.sigma_normals_points(x, rnd.feature_tables[b], rnd.resolution[b], rnd.params[b], ones,
                                                     axis_scale=[2.0 / s for s in sizes[b]], want_grad=True)
        evaluated += int(i.numel())
        num[i] += w[i] * sigma
        A[i] += w[i, None] * grad
        B[i] += sigma[:, None] * gw[i]
        hit[i] = True
    inv = torch.where(W > 0, 1.0 / W, torch.ones_like(W))
    v = num * inv
    g = ((A + B) - v[:, None] * C) * inv[:, None]
    return torch.where(hit, v, torch.zeros_like(v)), torch.where(hit[:, None], g, torch.zeros_like(g)), evaluated


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="256,512", help="lattice cells along the scene box's longest side, one mesh each")
    ap.add_argument("--log2-T", type=int, default=19)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_normals_bench.json"))
    args = ap.parse_args()
    import scanerf_amd  # noqa
    from scanerf_amd import meshing, render
    from bench_scene_mesh import build_scene
    dev = "cuda:0"
    rnd = build_scene(dev, args.log2_T)
    tiles = (rnd.feature_tables, rnd.resolution, rnd.params, rnd.block_corner, rnd.block_size, rnd.occupied_grid, rnd.grid_starts,
             rnd.grid_log2dim)
    corner, size = rnd.scene_box()
    x0 = meshing.lattice_positions([32, 32, 32], dev)
    sigma0, _, _ = render.sigma_normals_points(x0, rnd.feature_tables[0], rnd.resolution[0], rnd.params[0], torch.ones(32, device=dev))
    level = float(sigma0.median())
    out = {"device": torch.cuda.get_device_name(0), "tiles": int(rnd.feature_tables.shape[0]), "log2_T": args.log2_T, "table": "f16",
           "level": level, "box_corner": corner, "box_size": size, "occupancy": "sphere shell, radius 1.4, thickness 0.7, per tile", "runs": {}}
    fused = lambda p: meshing.scene_sigma_normals_points(p, *tiles, want_grad=True)
    for cells in (int(s) for s in args.cells.split(",")):
        n = meshing.cells_per_axis(size, cells)
        extract = lambda: meshing.extract_scene_mesh(*tiles, corner, size, n, level)
        mesh = extract()                                     # warm, and the vertices
        p = mesh.vertices
        perm = p[torch.randperm(p.shape[0], device=dev, generator=torch.Generator(device=dev).manual_seed(1))].contiguous()
        sf, gf, _ = fused(p)                                 # warm
        fused(perm)
        sc, gc, evaluated = composed(rnd, p)                 # warm
        scale = gf.norm(dim=1).clamp_min(1e-30)
        row = {"n": n, "V": int(p.shape[0]), "F": int(mesh.faces.shape[0]), "contributing_vertices": int((sf > 0).sum()),
               "composed_evaluated_points": evaluated,
               "composed_vs_fused_max_rel_grad_diff": float(((gc - gf).norm(dim=1) / scale)[sf > 0].max()) if bool((sf > 0).any()) else 0.0}
        pairs = []
        for _ in range(args.repeats):                        # alternating
            pairs.append({"fused_ms": clock(lambda: fused(p))[0], "composed_ms": clock(lambda: composed(rnd, p))[0],
                          "fused_permuted_ms": clock(lambda: fused(perm))[0], "extract_ms": clock(extract)[0]})
        med = {k: statistics.median(q[k] for q in pairs) for k in pairs[0]}
        row["alternating"] = pairs
        row["median_ms"] = med
        row["composed_over_fused"] = med["composed_ms"] / med["fused_ms"]
        row["permuted_over_brick_order"] = med["fused_permuted_ms"] / med["fused_ms"]
        row["fused_over_extract"] = med["fused_ms"] / med["extract_ms"]
        row["spread"] = {k: (max(q[k] for q in pairs) - min(q[k] for q in pairs)) / med[k] for k in pairs[0]}
        out["runs"][str(cells)] = row
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
