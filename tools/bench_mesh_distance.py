"""Cost of the closest-point query and of the mesh comparison built on it (csrc/mesh_distance.hip; FastMesh.closest_point,
evaluation.compare_meshes).

    python tools/bench_mesh_distance.py [--cells 256,512] [--large-n 1000] [--repeats 7] [--max-dist 0.5] [--out profiles/mesh_distance_bench.json]

pred: the scene meshes tools/bench_scene_mesh.py extracts (3 x 3 tiles, its level) at the given lattice sizes.  gt: the height field
of tools/bench_mesh.py (2 large_n^2 faces over [-10,10]^2).  The scene box (10 x 4 x 10 from (0,-2,0)) is mapped onto the height
field's frame -- (x, y, z) -> (2 x - 10, 2 z - 10, y / 2 + 1) -- so that pred lies within about two units of gt everywhere, as a
reconstruction lies near its scan; an evaluation of far-apart meshes is a different workload (see `far` below).

Per pred mesh and log2dim 6 and 7: points per second of the query for the mesh's vertices (lattice order) and for as many surface
samples (face order), uncut and with --max-dist; occupied cells looked at and face tests per point (the counting entry); one
`far` figure (the same vertices lifted by 4 units, uncut, a 65 536-point prefix) for the empty-space walk; the brute-force kernel on a
16 384-point prefix, compared with the grid route bit for bit; compare_meshes as a whole (build of both structures, sampling, both
queries, reductions) beside the extraction of the same mesh.

Host clock around work that ends in a device synchronise; every shape is run once before it is timed; the shapes alternate `repeats`
times; medians with spread ((max - min) / median).  Writes one JSON document, rewritten after every mesh."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="256,512")
    ap.add_argument("--large-n", type=int, default=1000)
    ap.add_argument("--log2-T", type=int, default=19)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--max-dist", type=float, default=0.5)
    ap.add_argument("--compare-samples", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_distance_bench.json"))
    args = ap.parse_args()
    import scanerf_amd  # noqa
    from bench_mesh import height_field
    from bench_scene_mesh import build_scene, clock
    from scanerf_amd import _capi, evaluation, meshing, render
    from scanerf_amd.fastmesh import FastMesh
    dev = "cuda:0"
    rnd = build_scene(dev, args.log2_T)
    x0 = meshing.lattice_positions([32, 32, 32], dev)
    sigma0, _, _ = render.sigma_normals_points(x0, rnd.feature_tables[0], rnd.resolution[0], rnd.params[0], torch.ones(32, device=dev))
    level = float(sigma0.median())                         # tools/bench_scene_mesh.py's level
    gv, gf = height_field(args.large_n, dev)
    gt = {L: FastMesh.from_arrays(gv, gf, dev, log2dim=L) for L in (6, 7)}
    out = {"device": torch.cuda.get_device_name(0), "level": level, "gt": {"V": int(gv.shape[0]), "F": int(gf.shape[0]),
           "pregathered": {str(L): gt[L].tris is not None for L in gt}, "face_list_entries": {str(L): int(gt[L].cell_faces.shape[0]) for L in gt}},
           "max_dist": args.max_dist, "repeats": args.repeats, "runs": {}}
    to_gt = lambda v: torch.stack([2 * v[:, 0] - 10, 2 * v[:, 2] - 10, 0.5 * v[:, 1] + 1], 1).contiguous()

    def counted(mesh, pts):
        dist2 = torch.empty(len(pts), device=dev)
        face = torch.empty(len(pts), dtype=torch.int32, device=dev)
        cnt = torch.empty(len(pts), 2, dtype=torch.int32, device=dev)
        _capi.check(_capi.lib().scanerf_mesh_closest_point_counted(
            pts.data_ptr(), len(pts), mesh.vertices.data_ptr(), mesh.faces.data_ptr(), mesh.tris.data_ptr() if mesh.tris is not None else None,
            mesh.bitmask.data_ptr(), mesh.rank.data_ptr(), mesh.start_num.data_ptr(), mesh.cell_faces.data_ptr(), mesh.cell_box.data_ptr(),
            mesh.scene_info.data_ptr(), mesh.log2dim, float("inf"), dist2.data_ptr(), face.data_ptr(), None, cnt.data_ptr(), _capi.stream()),
            "counted")
        c = cnt.double()
        return {"cells_per_point": float(c[:, 0].mean()), "face_tests_per_point": float(c[:, 1].mean()),
                "face_tests_max": int(cnt[:, 1].max()), "cells_max": int(cnt[:, 0].max())}

    for cells in (int(s) for s in args.cells.split(",")):
        mesh = rnd.extract_mesh(level, cells)
        pv, pf = to_gt(mesh.vertices), mesh.faces
        N = int(pv.shape[0])
        samples, _ = evaluation.sample_surface(pv, pf, N, 0)
        far = (pv[:65536] + torch.tensor([0.0, 0.0, 4.0], device=dev)).contiguous()
        sub = pv[:16384].contiguous()
        steps = {"extract_ms": lambda: rnd.extract_mesh(level, cells),
                 "compare_meshes_ms": lambda: evaluation.compare_meshes((pv, pf), (gv, gf), args.compare_samples, [0.05], max_dist=args.max_dist,
                                                                        device=dev),
                 "brute_16384_ms": lambda: gt[6].closest_point(sub, route="brute", want_closest=False)}
        for L in (6, 7):
            m = gt[L]
            steps[f"vertices_L{L}_ms"] = lambda m=m: m.closest_point(pv, want_closest=False)
            steps[f"samples_L{L}_ms"] = lambda m=m: m.closest_point(samples, want_closest=False)
            steps[f"vertices_L{L}_cut_ms"] = lambda m=m: m.closest_point(pv, args.max_dist, want_closest=False)
            steps[f"samples_L{L}_cut_ms"] = lambda m=m: m.closest_point(samples, args.max_dist, want_closest=False)
            steps[f"far_65536_L{L}_ms"] = lambda m=m: m.closest_point(far, want_closest=False)
        first = {}
        for k, fn in steps.items():                       # every shape once before it is timed
            first[k] = clock(fn)[0]
            print(f"cells {cells}: first {k} {first[k]:.1f} ms", flush=True)
        a, b = gt[6].closest_point(sub, route="brute"), gt[7].closest_point(sub)
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b)), "grid and brute force differ"
        d_uncut = gt[6].closest_point(pv, want_closest=False)[0]
        runs = [{k: clock(fn)[0] for k, fn in steps.items()} for _ in range(args.repeats)]
        med = {k: statistics.median(r[k] for r in runs) for k in steps}
        rate = {k[:-3] + "_points_per_s": (65536 if k.startswith("far") else 16384 if k.startswith("brute") else N) / (med[k] * 1e-3)
                for k in steps if k.split("_")[0] in ("vertices", "samples", "far", "brute")}
        row = {"V": N, "F": int(pf.shape[0]), "first_run_ms": first, "alternating": runs, "median_ms": med,
               "spread": {k: (max(r[k] for r in runs) - min(r[k] for r in runs)) / med[k] for k in steps}, "points_per_s": rate,
               "compare_meshes_over_extract": med["compare_meshes_ms"] / med["extract_ms"],
               "distance": {"mean": float(d_uncut.mean()), "max": float(d_uncut.max()),
                            "share_within_max_dist": float((d_uncut <= args.max_dist).float().mean())},
               "census": {f"{name}_L{L}": counted(gt[L], pts) for L in (6, 7) for name, pts in (("vertices", pv), ("samples", samples), ("far", far))}}
        out["runs"][str(cells)] = row
        json.dump(out, open(args.out, "w"), indent=1)
        print(json.dumps({"cells": cells, "V": N, "median_ms": med, "points_per_s": rate, "census": row["census"]}), flush=True)
        del mesh, pv, pf, samples, far, sub, steps


if __name__ == "__main__":
    main()
