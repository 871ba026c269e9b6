"""Cost of tile allocation's view coverage: the fused kernel (scanerf_amd.allocation.view_coverage, csrc/coverage.hip) beside
the same counts composed from the ops that existed before it -- per camera torch rays, FastMesh.first_hit, ray_aabb_intersection_v2
into a [B,K,2] bounds tensor, a comparison and a sum (what the reference's preprocess/build_tiles.py:129-156 does).

    python tools/bench_tile_alloc.py [--repeat 10] [--warmup 2] [--mesh-n 500] [--cameras 64] [--out profiles/tile_alloc_bench.txt]

Scene: a procedural terrain of 2 * mesh_n^2 faces (default 500 000) over [-10,10]^2, `cameras` 1920 x 1080 cameras on a ring
looking across it, scale 4 (480 x 270 rays per camera), a 10 x 1 x 10 grid of tiles.  Each figure is the median of `repeat` runs
over ALL cameras after `warmup`, timed with device events.  Also reported: the bytes the composed path materialises per camera
(rays, depth, bounds, the comparison) and whether the two paths give the same counts."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def composed_counts(fmesh, ks, c2ws, H, W, centers, sizes, scale):
    """counts [K,C] from the ops as they were: one camera at a time, everything materialised."""
    from scanerf_amd.cuda import ray_aabb_intersection_v2
    dev = ks.device
    h, w = H // scale, W // scale
    K = centers.shape[0]
    counts = torch.zeros(K, ks.shape[0], dtype=torch.int32, device=dev)
    j, i = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
    for c in range(ks.shape[0]):
        k = ks[c] / scale
        x, y = (i - k[0, 2]) / k[0, 0], (j - k[1, 2]) / k[1, 1]
        R = c2ws[c, :3, :3]
        d = (x[..., None] * R[:, 0] + y[..., None] * R[:, 1] + R[:, 2]).reshape(-1, 3).contiguous()
        o = c2ws[c, :3, 3].expand_as(d).contiguous()
        bounds = torch.full((d.shape[0], K, 2), -1.0, dtype=torch.float32, device=dev)
        ray_aabb_intersection_v2(o, d, centers, sizes, bounds)
        near = bounds[..., 0]
        depth = fmesh.first_hit(o, d)[:, None]
        depth = torch.where(depth == 0, torch.full_like(depth, 1e5), depth)
        counts[:, c] = ((near != -1) & (near < depth)).sum(0)
    return counts


def composed_bytes_per_camera(H, W, K, scale):
    B = (H // scale) * (W // scale)
    return {"rays": 2 * B * 12, "depth": B * 4, "bounds": B * K * 8, "comparison": B * K, "total": B * (24 + 4 + 9 * K)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mesh-n", type=int, default=500)
    ap.add_argument("--cameras", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    import fastmesh_reference as FR
    import scanerf_amd  # noqa
    from bench_mesh import event_ms, height_field
    from scanerf_amd import allocation
    from scanerf_amd.fastmesh import FastMesh
    dev = "cuda:0"
    H, W, scale = 1080, 1920, 4
    V, F = height_field(args.mesh_n, dev)
    fm = FastMesh.from_arrays(V, F, dev)
    ks, c2ws = [], []
    for c in range(args.cameras):
        a = 2 * np.pi * c / args.cameras
        c2w, K = FR.look_at((8.5 * np.cos(a), 8.5 * np.sin(a), 3.0 + 0.02 * c), (3 * np.cos(a + 2.5), 3 * np.sin(a + 2.5), 0.0), H, W, 1400.0)
        ks.append(K)
        c2ws.append(c2w)
    ks, c2ws = torch.from_numpy(np.stack(ks)).to(dev), torch.from_numpy(np.stack(c2ws)).to(dev)
    # 10 x 1 x 10 tiles: the scene is z-up, so the single-tile axis of the reference's y-up scenes is laid along y here by size
    bound = fm.get_sceneinfo().cpu()
    ext = bound[3:] - bound[:3]
    size = torch.tensor([float(ext[0]) / 9.5, float(ext[1]) * 1.01, float(ext[2]) / 9.5])   # ceil(9.5) = 10 tiles along x and z
    corners, side = allocation.tile_grid(bound, size, 0.2, (0.0, 0.0, 0.0), (10, 1, 10))
    centers, sizes = (corners + size / 2).to(dev), size.to(dev)[None].expand(corners.shape[0], 3).contiguous()
    fused = lambda: allocation.view_coverage(fm, ks, c2ws, H, W, centers, sizes, scale)
    composed = lambda: composed_counts(fm, ks, c2ws, H, W, centers, sizes, scale)
    assert side == [10, 1, 10], side
    a, b = fused(), composed()
    res = {"device": torch.cuda.get_device_name(0), "faces": int(F.shape[0]), "cameras": args.cameras, "frame": [H, W], "scale": scale,
           "rays_per_camera": (H // scale) * (W // scale), "tiles": side, "boxes": int(corners.shape[0]), "repeat": args.repeat,
           "pregathered": fm.tris is not None,
           "fused_ms": round(event_ms(fused, args.repeat, args.warmup), 3),
           "composed_ms": round(event_ms(composed, args.repeat, args.warmup), 3),
           "composed_bytes_per_camera": composed_bytes_per_camera(H, W, corners.shape[0], scale),
           "fused_bytes_written": int(a.numel() * 4),
           "entries_that_differ": int((a != b).sum()), "entries": int(a.numel()), "covered_share": round(float((a > 0).float().mean()), 3),
           "largest_count_share_of_a_frame": round(float(a.max()) / ((H // scale) * (W // scale)), 3)}
    res["speedup"] = round(res["composed_ms"] / res["fused_ms"], 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"tools/bench_tile_alloc.py --repeat {args.repeat} --warmup {args.warmup} --mesh-n {args.mesh_n} --cameras {args.cameras}\n")
            f.write(line + "\n")


if __name__ == "__main__":
    main()
