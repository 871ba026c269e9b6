"""Cost of rendering a mesh through cameras (csrc/mesh_render.hip): one 1920 x 1080 view and 32 views of 270 x 480, on
the terrain fixture of tests/fastmesh_reference.py (4 752 faces) and on the fused mesh of tools/bench_tsdf_fusion.py's scene (3 x 3 tiles,
`--cameras` views at 1 / `--scale`, `--cells` lattice cells, gradient normals and fused colours), at log2dim 6 and 7:

  * FastMesh.render_views `fused` with normals and colours, and with depth and face alone (what the attribute gathers cost);
  * the `composed` route (compute_ray_forward on a locs grid, trace, one torch op per operation), compared with the fused one BIT FOR BIT
    before anything is timed;
  * first_hit alone on materialised image-order rays -- the op from before this change -- and compute_ray_forward alone: the claim to
    test is fused <= first_hit on stored rays + the ray generation;
  * trace on the same stored rays (the hit record without the 8 x 8 mapping).

    python tools/bench_mesh_render.py [--cells 256] [--cameras 32] [--scale 4] [--repeats 9] [--out profiles/mesh_render_bench.txt]

Host clock around work that ends in a device synchronise; every shape runs once before it is timed; medians.  Not measured: kernel
times from a profiler run, hardware counters, a real capture's mesh."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("k_render_viewsILb1E", "k_render_viewsILb0E", "k_traceILb1E", "k_traceILb0E", "k_trace_brute", "k_first_hitILb0ELb1E")
SHAPES = ((1, 1080, 1920), (32, 270, 480))


def image_rays(k9, c12, H, W):
    """Image-order rays of every camera, stored: ([C*H*W,3], [C*H*W,3]) and the locs grid they came from."""
    from scanerf_amd.cuda import compute_ray_forward
    dev, C = k9.device, k9.shape[0]
    cam = torch.arange(C, device=dev, dtype=torch.int32)[:, None, None].expand(C, H, W)
    py = torch.arange(H, device=dev, dtype=torch.int32)[None, :, None].expand(C, H, W)
    px = torch.arange(W, device=dev, dtype=torch.int32)[None, None, :].expand(C, H, W)
    locs = torch.stack([cam, px, py], -1).reshape(-1, 3).contiguous()
    o = torch.empty(locs.shape[0], 3, device=dev)
    d = torch.empty(locs.shape[0], 3, device=dev)
    compute_ray_forward(o, d, k9, c12, locs)
    return o, d, locs


def terrain_cameras(C, H, W):
    import fastmesh_reference as FR
    if C == 1:
        cams = [FR.look_at((14.0, -12.0, 9.0), (0.0, 0.0, 0.0), H, W, 0.73 * W)]
    else:
        cams = [FR.look_at((16.0 * np.cos(a), 16.0 * np.sin(a), 8.0), (0.0, 0.0, 0.0), H, W, 0.73 * W) for a in 0.2 + 2 * np.pi * np.arange(C) / C]
    return torch.from_numpy(np.stack([k for _, k in cams])), torch.from_numpy(np.stack([m for m, _ in cams]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=256)
    ap.add_argument("--cameras", type=int, default=32)
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--log2-T", type=int, default=19)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--composed-repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    import scanerf_amd  # noqa
    import fastmesh_reference as FR
    from bench_mesh_visibility import kernel_resources
    from bench_scene_mesh import build_scene, clock
    from bench_tsdf_fusion import ring
    from scanerf_amd import _capi
    from scanerf_amd.allocation import _cameras
    from scanerf_amd.cuda import compute_ray_forward
    from scanerf_amd.fastmesh import FastMesh
    dev = "cuda:0"
    med = lambda f, k: round(statistics.median([clock(f)[0] for _ in range(1 + k)][1:]), 4)
    res = {"device": torch.cuda.get_device_name(0), "kernels": {k: kernel_resources(_capi.LIB_PATH, k) for k in KERNELS}, "meshes": {}}

    meshes = {}
    V, F, _ = FR.terrain_fixture()
    rng = np.random.default_rng(24)
    meshes["terrain"] = dict(v=torch.from_numpy(V).to(dev), f=torch.from_numpy(F).to(dev),
                             n=torch.from_numpy(rng.normal(size=V.shape).astype(np.float32)).to(dev),
                             c=torch.from_numpy(rng.uniform(0, 1, V.shape).astype(np.float32)).to(dev), cameras=terrain_cameras)
    rnd = build_scene(dev, args.log2_T)
    corner, size = rnd.scene_box()
    center = [corner[k] + size[k] / 2 for k in range(3)]
    ks, c2ws = ring(center, 1.1 * max(size), 0.5 * max(size), args.cameras, 1080, 1920, 1400.0)
    fused_mesh, rgb = rnd.fuse_mesh((ks, c2ws, 1080, 1920), cells_per_axis=args.cells, scale=args.scale, colors="diffuse", normals=True)
    meshes["fused_scene"] = dict(v=fused_mesh.vertices, f=fused_mesh.faces, n=fused_mesh.normals.contiguous(), c=rgb.contiguous(),
                                 cameras=lambda C, H, W: ring(center, 1.1 * max(size), 0.5 * max(size), C, H, W, 0.73 * W))
    del rnd
    torch.cuda.empty_cache()

    for name, m in meshes.items():
        out = res["meshes"][name] = {"V": int(m["v"].shape[0]), "F": int(m["f"].shape[0]), "runs": {}}
        for log2dim in (6, 7):
            fm = FastMesh.from_arrays(m["v"], m["f"], dev, log2dim=log2dim)
            for C, H, W in SHAPES:
                kc, cc = m["cameras"](C, H, W)
                k9, c12 = _cameras(kc, cc, dev)
                k3, c34 = k9.reshape(-1, 3, 3), c12.reshape(-1, 3, 4)
                full = lambda route="fused": fm.render_views(k3, c34, H, W, normals=m["n"], colors=m["c"], route=route)
                a, b = full(), full("composed")
                same = all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a) and set(a) == set(b)
                hit_share = float((a["face"] >= 0).float().mean())
                del a, b
                o, d, locs = image_rays(k9, c12, H, W)
                oo, dd = torch.empty_like(o), torch.empty_like(d)
                depth = torch.empty(o.shape[0], device=dev)
                row = {"pixels": C * H * W, "hit_share": round(hit_share, 4), "fused_equals_composed_in_every_bit": same,
                       "fused_normals_colors_ms": med(full, args.repeats),
                       "fused_depth_face_ms": med(lambda: fm.render_views(k3, c34, H, W), args.repeats),
                       "composed_ms": med(lambda: full("composed"), args.composed_repeats) if args.composed_repeats else None,
                       "first_hit_stored_rays_ms": med(lambda: fm.first_hit(o, d, out=depth), args.repeats),
                       "trace_stored_rays_ms": med(lambda: fm.trace(o, d), args.repeats),
                       "ray_generation_ms": med(lambda: compute_ray_forward(oo, dd, k9, c12, locs), args.repeats)}
                row["fused_depth_face_over_first_hit_plus_rays"] = round(
                    row["fused_depth_face_ms"] / (row["first_hit_stored_rays_ms"] + row["ray_generation_ms"]), 3)
                row["fused_normals_colors_over_first_hit_plus_rays"] = round(
                    row["fused_normals_colors_ms"] / (row["first_hit_stored_rays_ms"] + row["ray_generation_ms"]), 3)
                out["runs"][f"log2dim={log2dim},{C}x{H}x{W}"] = row
                del o, d, locs, oo, dd, depth
            del fm
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"tools/bench_mesh_render.py --cells {args.cells} --cameras {args.cameras} --scale {args.scale} --repeats {args.repeats} "
                    f"--composed-repeats {args.composed_repeats}\n")
            f.write(line + "\n")


if __name__ == "__main__":
    main()
