"""Cost of the project-and-blend op: the fused kernel (FastMesh.project_colors, csrc/mesh_colors.hip) beside the same
answer composed from the ops that existed before it (route="composed": per camera the frustum test as torch elementwise ops,
FastMesh.first_hit on the pairs in view, then the sample and the blend as torch elementwise ops), and beside point_views alone on the
same inputs (the geometric half, fused and composed).

    python tools/bench_mesh_colors.py [--repeat 10] [--warmup 2] [--mesh-n 350] [--cameras 32] [--out profiles/mesh_colors_bench.txt]

Two scenes, one JSON line each:
  terrain   the tests' terrain (2 497 vertices, 4 752 faces) against its 8 cameras at 102 x 134: the size of the test suite, a
            measurement of overheads;
  large     the procedural terrain of tools/bench_mesh.py (2 * mesh_n^2 faces, default 245 000, 123 201 vertices) against `cameras`
            1080 x 1920 cameras on the ring of tools/bench_mesh_visibility.py, random images, the mesh's own vertex normals, bias = half
            the mean edge.
Each time is the median of `repeat` runs over ALL cameras after `warmup`, timed with device events, all routes in this one process,
alternating.  Also reported: pairs per second, the occupied cells and ray / triangle tests per pair in view and the share of the
pairs that contributed (the counted entry), the kernel's registers / LDS / scratch, whether the routes give the same bits, and the
one expectation stated for this kernel: fused_ms <= point_views_ms + (composed_ms - point_views_composed_ms), i.e. the fused route is
not slower than the fused geometric half plus the composed sampling.  Not measured: other camera counts, log2dim 7, real captures."""
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


def counted(fm, pts, nrm, img, ks, c2ws, bias, min_cos):
    """-> (acc, count, [pairs in view, occupied cells looked at, ray / triangle tests, pairs that contributed]) from the counted entry."""
    from scanerf_amd import _capi
    from scanerf_amd.allocation import _cameras
    k9, c12 = _cameras(ks, c2ws, pts.device)
    N = pts.shape[0]
    acc = torch.zeros(N, 4, dtype=torch.float32, device=pts.device)
    count = torch.zeros(N, dtype=torch.int32, device=pts.device)
    counters = torch.zeros(4, dtype=torch.int64, device=pts.device)
    p = lambda t: None if t is None else t.data_ptr()
    _capi.check(_capi.tool("scanerf_mesh_project_colors_counted")(
        p(pts), p(nrm), N, p(img), p(k9), p(c12), k9.shape[0], img.shape[1], img.shape[2], bias, 0.0, float("inf"), min_cos, p(fm.vertices),
        p(fm.faces), p(fm.tris), p(fm.bitmask), p(fm.rank), p(fm.start_num), p(fm.cell_faces), p(fm.scene_info), fm.log2dim, p(acc), p(count),
        p(counters), _capi.stream()), "mesh_project_colors_counted")
    return acc, count, counters.tolist()


def measure(name, fm, pts, nrm, img, ks, c2ws, bias, min_cos, repeat, warmup):
    from bench_mesh import event_ms
    from bench_mesh_visibility import kernel_resources
    from scanerf_amd import _capi
    H, W = int(img.shape[1]), int(img.shape[2])
    kw = dict(normals=nrm, min_cos=min_cos)
    fused = lambda: fm.project_colors(pts, img, ks, c2ws, bias, **kw)
    composed = lambda: fm.project_colors(pts, img, ks, c2ws, bias, route="composed", **kw)
    views = lambda: fm.point_views(pts, ks, c2ws, H, W, bias, want_mask=True)
    views_composed = lambda: fm.point_views(pts, ks, c2ws, H, W, bias, want_mask=True, route="composed")
    (a, ac), (b, bc) = fused(), composed()
    cacc, ccount, (walked, cells, tests, used) = counted(fm, pts, nrm, img, ks, c2ws, bias, min_cos)
    seen = int(views()[0].sum())
    times = {k: [] for k in ("fused_ms", "composed_ms", "point_views_ms", "point_views_composed_ms")}
    for _ in range(3):      # the routes alternate: three rounds of `repeat` runs each, the median of the three medians is reported
        for k, fn in zip(times, (fused, composed, views, views_composed)):
            times[k].append(event_ms(fn, repeat, warmup))
    pairs = int(pts.shape[0]) * int(ks.shape[0])
    res = {"scene": name, "device": torch.cuda.get_device_name(0), "faces": int(fm.faces.shape[0]), "points": int(pts.shape[0]),
           "cameras": int(ks.shape[0]), "frame": [H, W], "log2dim": fm.log2dim, "pregathered": fm.tris is not None, "bias": round(bias, 5),
           "min_cos": min_cos, "repeat": repeat}
    res.update({k: round(float(np.median(v)), 3) for k, v in times.items()})
    res.update({k.replace("_ms", "_ms_rounds"): [round(x, 3) for x in v] for k, v in times.items()})
    res.update(pairs=pairs, pairs_in_view=walked, share_in_view=round(walked / pairs, 4), pairs_seen=seen, pairs_contributed=used,
               share_contributed=round(used / pairs, 4), share_of_seen_contributed=round(used / max(seen, 1), 4),
               points_without_a_colour=int((ac == 0).sum()), cells_per_pair_in_view=round(cells / max(walked, 1), 2),
               tests_per_pair_in_view=round(tests / max(walked, 1), 2),
               acc_rows_that_differ=int((a.view(torch.int32) != b.view(torch.int32)).any(1).sum()), counts_that_differ=int((ac != bc).sum()),
               counted_entry_agrees=bool(torch.equal(cacc.view(torch.int32), a.view(torch.int32)) and torch.equal(ccount, ac)),
               kernel=kernel_resources(_capi.LIB_PATH, "k_project_colorsILb1ELb0"))
    res["pairs_per_s"] = round(pairs / res["fused_ms"] * 1e3)
    res["speedup_over_composed"] = round(res["composed_ms"] / res["fused_ms"], 2)
    res["composed_sampling_ms"] = round(res["composed_ms"] - res["point_views_composed_ms"], 3)
    res["fused_over_point_views"] = round(res["fused_ms"] / res["point_views_ms"], 3)
    res["not_slower_than_point_views_plus_composed_sampling"] = bool(res["fused_ms"] <= res["point_views_ms"] + res["composed_sampling_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mesh-n", type=int, default=350)
    ap.add_argument("--cameras", type=int, default=32)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    import fastmesh_reference as FR
    import mesh_colors_reference as MC
    import scanerf_amd  # noqa
    from bench_mesh import height_field
    from scanerf_amd.fastmesh import FastMesh
    dev = "cuda:0"
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    lines = []
    case = MC.terrain()
    fm = FastMesh.from_arrays(case["V"], case["F"], dev)
    lines.append(measure("terrain", fm, t(case["points"]), t(case["normals"]), t(case["random"]), t(case["ks"]), t(case["c2ws"]), case["bias"],
                         case["min_cos"], args.repeat, args.warmup))
    H, W = 1080, 1920
    V, F = height_field(args.mesh_n, dev)
    fm = FastMesh.from_arrays(V, F, dev)
    ks, c2ws = [], []
    for c in range(args.cameras):
        a = 2 * np.pi * c / args.cameras
        c2w, K = FR.look_at((8.5 * np.cos(a), 8.5 * np.sin(a), 3.0 + 0.02 * c), (3 * np.cos(a + 2.5), 3 * np.sin(a + 2.5), 0.0), H, W, 1400.0)
        ks.append(K)
        c2ws.append(c2w)
    ks, c2ws = t(np.stack(ks).astype(np.float32)), t(np.stack(c2ws).astype(np.float32))
    tri = fm.vertices[fm.faces.long()]
    edges = torch.cat([(tri[:, 1] - tri[:, 0]).norm(dim=1), (tri[:, 2] - tri[:, 1]).norm(dim=1), (tri[:, 0] - tri[:, 2]).norm(dim=1)])
    bias = 0.5 * float(edges.mean())
    n = torch.zeros_like(fm.vertices).index_add_(0, fm.faces.long().reshape(-1),
                                                 torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).repeat_interleave(3, 0))
    n = n / n.norm(dim=1, keepdim=True).clamp_min(1e-20)
    n = torch.where(n[:, 2:3] < 0, -n, n).contiguous()      # the cameras are above the terrain
    img = torch.rand(args.cameras, H, W, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    lines.append(measure("large", fm, fm.vertices, n, img, ks, c2ws, bias, 0.0, args.repeat, args.warmup))
    text = "\n".join(json.dumps(r) for r in lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"tools/bench_mesh_colors.py --repeat {args.repeat} --warmup {args.warmup} --mesh-n {args.mesh_n} --cameras {args.cameras}\n")
            f.write(text + "\n")


if __name__ == "__main__":
    main()
