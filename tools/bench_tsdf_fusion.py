"""Cost of the depth-map fusion (csrc/tsdf.hip, scanerf_amd/fusion.py) on the scene of tools/bench_scene_mesh.py
(3 x 3 tiles, T = 2^19 f16, sphere-shell occupancies), whose cameras here are a ring of `--cameras` 1080 x 1920 views around it
rendered at 1 / `--scale` (a synthetic scene has no capture):

  * the depth renders (TileSetRenderer.render + fusion.mask_depth), all cameras, once: they dominate a fuse_mesh call;
  * per lattice (`--cells` along the box's longest side): TSDFVolume.integrate over all cameras, `fused` (one launch) beside
    `composed` (the torch witness, one eager op per operation, no skip), compared BIT FOR BIT before anything is timed; the counted
    entry's pairs evaluated, (block, camera) pairs skipped and updates; bytes per second on acc (every row read, the updated rows
    written) and on the depth maps (their size, each read at least once); values + extraction (surface nets, support, cull, filter);
    the fused mesh's component count and the largest component's share of the vertices, next to the level-set mesh of the same
    scene on the same lattice (meshing.extract_scene_mesh at bench_scene_mesh's level);
  * the colour route on the same maps with the renders' clamped diffuse images: `fused` with colour beside
    `composed` with colour, compared bit for bit in acc and cacc first, acc against the plain entry's; the counted entry's coloured
    pairs; the time as a ratio to the plain kernel's of the same visit; vertex_colors on the extracted mesh; bytes held.

    python tools/bench_tsdf_fusion.py [--cells 256,512] [--cameras 32] [--scale 4] [--repeats 5] [--composed-repeats 2]
                                      [--out profiles/tsdf_fusion_bench.txt]

Host clock around work that ends in a device synchronise; every shape runs once before it is timed; medians.  Not measured: a real
capture's cameras, other trunc values than the default, min_weight > 1."""
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


def ring(center, radius, height, n, H, W, focal):
    """n cameras on a circle around the y axis through `center` (the scene's tiles lie in the xz plane), `height` above it, looking at
    the centre: columns right, down, forward, eye (right x down = forward)."""
    ks, c2ws = [], []
    for a in 0.2 + 2 * np.pi * np.arange(n) / n:
        eye = np.asarray(center, float) + np.array([radius * np.cos(a), height, radius * np.sin(a)])
        fwd = (np.asarray(center, float) - eye) / np.linalg.norm(np.asarray(center, float) - eye)
        right = np.cross(fwd, [0.0, 1.0, 0.0])
        right /= np.linalg.norm(right)
        c2ws.append(np.stack([right, np.cross(fwd, right), fwd, eye], 1).astype(np.float32))
        ks.append(np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1.0]], np.float32))
    return torch.from_numpy(np.stack(ks)), torch.from_numpy(np.stack(c2ws))


def largest_share(mesh):
    from scanerf_amd import meshing
    V = int(mesh.vertices.shape[0])
    if V == 0:
        return 0, 0.0
    comps = meshing.mesh_components(mesh.faces, V)
    return int(comps.label.shape[0]), float(comps.n_vertices.max()) / V


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="256,512")
    ap.add_argument("--cameras", type=int, default=32)
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--log2-T", type=int, default=19)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--composed-repeats", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    args = ap.parse_args()
    import scanerf_amd  # noqa
    from bench_mesh_visibility import kernel_resources
    from bench_scene_mesh import build_scene, clock
    from scanerf_amd import _capi, fusion, meshing, render
    dev = "cuda:0"
    rnd = build_scene(dev, args.log2_T)
    corner, size = rnd.scene_box()
    center = [corner[k] + size[k] / 2 for k in range(3)]
    H, W = 1080, 1920
    ks, c2ws = ring(center, 1.1 * max(size), 0.5 * max(size), args.cameras, H, W, 1400.0)
    h, w = H // args.scale, W // args.scale
    k2 = fusion.scale_cameras(ks, args.scale).to(dev)
    c2ws = c2ws.to(dev)

    def renders(images=None):
        maps = []
        for K, c2w in zip(k2, c2ws):
            diffuse, _, depth, transp = rnd.render(h, w, K, c2w)
            maps.append(fusion.mask_depth(depth[..., 0], transp[..., 0], 0.5))
            if images is not None:
                images.append(fusion.clamped_image(diffuse))
        return torch.stack(maps).contiguous()

    renders()                                           # warm
    render_ms, maps = clock(renders)
    images = []
    renders(images)
    images = torch.stack(images).contiguous()
    x0 = meshing.lattice_positions([32, 32, 32], dev)
    sigma0, _, _ = render.sigma_normals_points(x0, rnd.feature_tables[0], rnd.resolution[0], rnd.params[0], torch.ones(32, device=dev))
    level = float(sigma0.median())
    res = {"device": torch.cuda.get_device_name(0), "tiles": int(rnd.feature_tables.shape[0]), "cameras": args.cameras, "frame": [h, w],
           "scale": args.scale, "pixels_with_depth": round(float((maps > 0).float().mean()), 4), "render_all_cameras_ms": round(render_ms, 1),
           "cameras_per_pass": int(_capi.tool("scanerf_tsdf_cameras_per_pass")()), "kernel": kernel_resources(_capi.LIB_PATH, "k_tsdf_integrateILb0ELb0"),
           "kernel_color": kernel_resources(_capi.LIB_PATH, "k_tsdf_integrateILb0ELb1"),
           "kernel_vertex_colors": kernel_resources(_capi.LIB_PATH, "k_tsdf_vertex_colors"),
           "level_of_the_level_set": level, "runs": {}}
    for cells in (int(s) for s in args.cells.split(",")):
        n = meshing.cells_per_axis(size, cells)
        spacing = fusion.lattice_spacing(size, n)
        new = lambda: fusion.TSDFVolume(corner, spacing, n, fusion.default_trunc(spacing), dev)
        vol = new()
        P = vol.points
        a = new().integrate(maps, k2, c2ws).acc
        b = new().integrate(maps, k2, c2ws, route="composed").acc
        differ = int((a.view(torch.int32) != b.view(torch.int32)).any(1).sum())
        del b
        counters = torch.zeros(3, dtype=torch.int64, device=dev)
        c = new().integrate(maps, k2, c2ws, counters=counters).acc
        counted_agrees = bool(torch.equal(a.view(torch.int32), c.view(torch.int32)))
        del c
        pairs, skipped, updates = counters.tolist()
        touched = int((a[:, 1] > 0).sum())

        def timed(route, repeats):
            out = []
            for _ in range(repeats):
                vol.acc.zero_()
                out.append(clock(lambda: vol.integrate(maps, k2, c2ws, route=route))[0])
            return out
        fused_ms, composed_ms = timed("fused", args.repeats), timed("composed", args.composed_repeats)
        vol.acc.copy_(a)
        extract_ms = [clock(lambda: vol.extract(report={}))[0] for _ in range(1 + args.repeats)][1:]
        report = {}
        mesh = vol.extract(report=report)
        n_comp, share = largest_share(mesh)
        ls = rnd.extract_mesh(level, cells)
        ls_comp, ls_share = largest_share(ls)
        fm = statistics.median(fused_ms)
        tiles = int(np.prod([-(-(n[0] + 1) // 2), -(-(n[1] + 1) // 2), -(-(n[2] + 1) // 64)]))
        res["runs"][str(cells)] = {
            "n": n, "points": P, "trunc": vol.trunc, "points_that_differ_fused_vs_composed": differ, "counted_entry_agrees": counted_agrees,
            "fused_ms": [round(v, 3) for v in fused_ms], "composed_ms": [round(v, 1) for v in composed_ms],
            "fused_median_ms": round(fm, 3), "composed_over_fused": round(statistics.median(composed_ms) / fm, 1),
            "pairs": P * args.cameras, "pairs_evaluated": pairs, "share_of_pairs_skipped": round(1.0 - pairs / (P * args.cameras), 4),
            "block_camera_pairs_skipped": skipped, "block_camera_pairs": tiles * args.cameras, "updates": updates,
            "pairs_evaluated_per_s": round(pairs / fm * 1e3), "points_observed": touched,
            "acc_bytes_per_s": round((P * 8 + touched * 8) / fm * 1e3), "depth_map_bytes_per_s": round(maps.numel() * 4 / fm * 1e3),
            "values_and_extraction_ms": round(statistics.median(extract_ms), 2),
            "fused_mesh": {"V": int(mesh.vertices.shape[0]), "F": int(mesh.faces.shape[0]), "raw_V": report["support"]["vertices"][0],
                           "components": n_comp, "largest_component_share_of_vertices": round(share, 4)},
            "level_set_mesh": {"V": int(ls.vertices.shape[0]), "F": int(ls.faces.shape[0]), "components": ls_comp,
                               "largest_component_share_of_vertices": round(ls_share, 4)}}
        # ---- the colour route: same maps, the renders' clamped diffuse images
        newc = lambda: fusion.TSDFVolume(corner, spacing, n, fusion.default_trunc(spacing), dev, color=True)
        fc = newc().integrate(maps, k2, c2ws, colors=images)
        cc = newc().integrate(maps, k2, c2ws, route="composed", colors=images)
        bits = lambda t: t.view(torch.int32)
        color_differ = int(((bits(fc.acc) != bits(cc.acc)).any(1) | (bits(fc.cacc) != bits(cc.cacc)).any(1)).sum())
        acc_agrees = bool(torch.equal(bits(fc.acc), bits(a)))
        del cc
        counters4 = torch.zeros(4, dtype=torch.int64, device=dev)
        newc().integrate(maps, k2, c2ws, counters=counters4, colors=images)
        volc = newc()

        def timed_color(route, repeats):
            out = []
            for _ in range(repeats):
                volc.acc.zero_()
                volc.cacc.zero_()
                out.append(clock(lambda: volc.integrate(maps, k2, c2ws, route=route, colors=images))[0])
            return out
        timed_color("fused", 1)
        color_ms, color_composed_ms = timed_color("fused", args.repeats), timed_color("composed", args.composed_repeats)
        plain_again_ms = timed("fused", args.repeats)      # the plain kernel again, after the colour runs: the same visit's spread
        vc_ms = [clock(lambda: fc.vertex_colors(mesh))[0] for _ in range(1 + args.repeats)][1:]
        rgb, weight = fc.vertex_colors(mesh)
        cm = statistics.median(color_ms)
        coloured_points = int((fc.cacc[:, 3] > 0).sum())
        res["runs"][str(cells)]["color"] = {
            "points_that_differ_fused_vs_composed": color_differ, "acc_equals_the_plain_entry": acc_agrees,
            "fused_ms": [round(v, 3) for v in color_ms], "composed_ms": [round(v, 1) for v in color_composed_ms],
            "fused_median_ms": round(cm, 3), "composed_over_fused": round(statistics.median(color_composed_ms) / cm, 1),
            "plain_fused_ms_after": [round(v, 3) for v in plain_again_ms],
            "color_over_plain": round(cm / statistics.median(fused_ms + plain_again_ms), 3),
            "counters": counters4.tolist(), "coloured_share_of_updates": round(counters4[3].item() / max(1, counters4[2].item()), 4),
            "points_coloured": coloured_points, "cacc_bytes_per_s": round((P * 16 + coloured_points * 16) / cm * 1e3),
            "image_bytes": images.numel() * 4, "vertex_colors_ms": round(statistics.median(vc_ms), 3),
            "vertices_uncoloured": int((weight == 0).sum()), "bytes_held": {"acc": P * 8, "cacc": P * 16, "images_per_view": h * w * 12}}
        del a, vol, mesh, ls, fc, volc, rgb, weight
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write(f"tools/bench_tsdf_fusion.py --cells {args.cells} --cameras {args.cameras} --scale {args.scale} --repeats {args.repeats} "
                    f"--composed-repeats {args.composed_repeats}\n")
            f.write(line + "\n")


if __name__ == "__main__":
    main()
