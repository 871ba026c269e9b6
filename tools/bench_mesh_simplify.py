"""Cost of mesh simplification by vertex clustering (csrc/mesh_simplify.hip) on the scene and cameras of
tools/bench_tsdf_fusion.py (3 x 3 tiles, a ring of `--cameras` views rendered at 1 / `--scale`), per lattice (`--cells` along the
box's longest side), on the mesh TSDFVolume.extract(normals=True) returns, at cluster cells of `--spacings` lattice spacings:

  * meshing.simplify_mesh `fused` beside `composed` (the torch witness), compared BIT FOR BIT before anything is timed; the fused
    call with the normals and without any attribute; the two entries (cluster pass, emit pass) on their own;
  * V -> V', F -> F', the largest cluster; the integer atomics of the sum pass per call (a count + 3 position sums + 3 per attribute,
    per vertex) and the bytes the passes ask for per vertex;
  * values + extraction (the step it follows) in the same visit;
  * evaluation.compare_meshes(simplified, original): accuracy and completeness in units of the cluster cell (a measurement).

    python tools/bench_mesh_simplify.py [--cells 256,512] [--spacings 2,4] [--cameras 32] [--scale 4] [--repeats 9]
                                        [--composed-repeats 3] [--samples 200000] [--out profiles/mesh_simplify_bench.txt]

Host clock around work that ends in a device synchronise; every shape runs once before it is timed; medians.  Kernel times come from
a `rocprofv3 --kernel-trace --stats` run of this script, on its own (appended to the file by hand).  Not measured: hardware counters,
a real capture's mesh."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("k_insert", "k_labels", "k_root_rows", "k_vertex_rows", "k_count_faces", "k_accumulate", "k_finalise", "k_emit_faces")


def entries(mesh, h, dev):
    """-> (cluster(), emit()): the two entries on buffers allocated once, for timing them alone."""
    from scanerf_amd import _capi
    V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    nbytes = ctypes.c_size_t(0)
    _capi.check(_capi.tool("scanerf_mesh_simplify_scratch_bytes")(V, F, ctypes.addressof(nbytes)), "mesh_simplify_scratch_bytes")
    scratch = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
    origin = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    nrm = None if mesh.normals is None else mesh.normals.data_ptr()
    head = (mesh.vertices.data_ptr(), mesh.faces.data_ptr(), nrm, None, V, F, ctypes.addressof(origin), float(h), scratch.data_ptr(),
            int(nbytes.value))
    st = lambda: torch.cuda.current_stream().cuda_stream
    cluster = lambda: _capi.check(_capi.tool("scanerf_mesh_simplify_cluster")(*head, st()), "mesh_simplify_cluster")
    cluster()
    Vk, Fk, _ = scratch[:24].view(torch.int64).tolist()
    new = lambda rows, cols, dt: torch.empty((rows, cols), dtype=dt, device=dev)
    sums, counts, ov, of = new(Vk, 9, torch.int64), new(Vk, 1, torch.int32), new(Vk, 3, torch.float32), new(max(Fk, 1), 3, torch.int32)
    on = None if nrm is None else new(Vk, 3, torch.float32)
    keep = (scratch, origin, sums, counts, ov, of, on)
    emit = lambda: _capi.check(_capi.tool("scanerf_mesh_simplify_emit")(*head, sums.data_ptr(), counts.data_ptr(), ov.data_ptr(), of.data_ptr(),
                                                                        None if on is None else on.data_ptr(), None, Vk, Fk, st()),
                               "mesh_simplify_emit") and keep
    return cluster, emit, int(nbytes.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="256,512")
    ap.add_argument("--spacings", default="2,4", help="cluster cells, in lattice spacings")
    ap.add_argument("--cameras", type=int, default=32)
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--log2-T", type=int, default=19)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--composed-repeats", type=int, default=3)
    ap.add_argument("--samples", type=int, default=200000, help="compare_meshes samples per surface (0: skip the comparison)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    args = ap.parse_args()
    import scanerf_amd  # noqa
    from bench_mesh_visibility import kernel_resources
    from bench_scene_mesh import build_scene, clock
    from bench_tsdf_fusion import ring
    from scanerf_amd import _capi, evaluation, fusion, meshing
    dev = "cuda:0"
    rnd = build_scene(dev, args.log2_T)
    corner, size = rnd.scene_box()
    center = [corner[k] + size[k] / 2 for k in range(3)]
    H, W = 1080, 1920
    ks, c2ws = ring(center, 1.1 * max(size), 0.5 * max(size), args.cameras, H, W, 1400.0)
    h_img, w_img = H // args.scale, W // args.scale
    k2 = fusion.scale_cameras(ks, args.scale).to(dev)
    c2ws = c2ws.to(dev)
    maps = []
    for K, c2w in zip(k2, c2ws):
        _, _, depth, transp = rnd.render(h_img, w_img, K, c2w)
        maps.append(fusion.mask_depth(depth[..., 0], transp[..., 0], 0.5))
    maps = torch.stack(maps).contiguous()
    res = {"device": torch.cuda.get_device_name(0), "tiles": int(rnd.feature_tables.shape[0]), "cameras": args.cameras,
           "kernels": {k: kernel_resources(_capi.LIB_PATH, k + "E") for k in KERNELS}, "runs": {}}
    bits = lambda t: t.view(torch.int32)
    med = lambda f, k: statistics.median([clock(f)[0] for _ in range(1 + k)][1:])
    for cells in (int(s) for s in args.cells.split(",")):
        n = meshing.cells_per_axis(size, cells)
        spacing = fusion.lattice_spacing(size, n)
        vol = fusion.TSDFVolume(corner, spacing, n, fusion.default_trunc(spacing), dev)
        vol.integrate(maps, k2, c2ws)
        mesh = vol.extract(normals=True)
        bare = mesh._replace(normals=None)
        V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
        extract_ms = med(lambda: vol.extract(), args.repeats)
        run = res["runs"][str(cells)] = {"n": n, "V": V, "F": F, "values_and_extraction_ms": round(extract_ms, 3), "cells": {}}
        for mult in (float(s) for s in args.spacings.split(",")):
            h = mult * max(spacing)
            report = {}
            fused = meshing.simplify_mesh(mesh, h, report=report)
            composed = meshing.simplify_mesh(mesh, h, route="composed")
            same = all(a.shape == b.shape and bool((bits(a) == bits(b)).all()) for a, b in
                       ((fused.vertices, composed.vertices), (fused.faces, composed.faces), (fused.normals, composed.normals)))
            del composed
            call_ms = med(lambda: meshing.simplify_mesh(mesh, h), args.repeats)
            bare_ms = med(lambda: meshing.simplify_mesh(bare, h), args.repeats)
            composed_ms = med(lambda: meshing.simplify_mesh(mesh, h, route="composed"), args.composed_repeats) if args.composed_repeats else None
            cluster, emit, scratch_bytes = entries(mesh, h, dev)
            cluster_ms, emit_ms = med(cluster, args.repeats), med(emit, args.repeats)
            Vk, Fk = report["vertices"][1], report["faces"][1]
            row = {"h": h, "h_in_spacings": mult, "V_out": Vk, "F_out": Fk, "largest_cluster": report["largest_cluster"],
                   "fused_equals_composed_in_every_bit": same, "simplify_mesh_ms": round(call_ms, 4), "without_attributes_ms": round(bare_ms, 4),
                   "composed_ms": composed_ms and round(composed_ms, 2), "composed_over_fused": composed_ms and round(composed_ms / call_ms, 1),
                   "cluster_entry_ms": round(cluster_ms, 4), "emit_entry_ms": round(emit_ms, 4),
                   "call_over_extraction": round(call_ms / extract_ms, 3), "scratch_bytes": scratch_bytes,
                   "scratch_bytes_per_vertex": round(scratch_bytes / V, 1), "sum_pass_atomics": V * 7,
                   # insert: 12 (+12 normals) read, 4 slot written; labels, root_rows, vertex_rows: 4 + 4, 4 + 4, 4 + 4 + 4;
                   # accumulate: 12 + 12 + 4 read, 7 atomics of 8 / 4 bytes; faces: 12 read twice, 3 x 4 gathered twice
                   "bytes_asked_per_vertex": {"cluster_pass": 24 + 4 + 8 + 8 + 12, "sum_pass_reads": 28, "sum_pass_atomic_bytes": 6 * 8 + 4,
                                              "per_face_both_passes": 2 * (12 + 12)}}
            if args.samples:
                sc = evaluation.compare_meshes((fused.vertices, fused.faces), (mesh.vertices, mesh.faces), args.samples, (h,), device=dev)
                # accuracy: simplified -> original (pred_to_gt); completeness: original -> simplified (gt_to_pred); mean and max, in h
                row["compare_meshes_in_h"] = {name: {k: round(float(sc[way][k]) / h, 4) for k in ("mean", "max") if k in sc[way]}
                                              for name, way in (("accuracy", "pred_to_gt"), ("completeness", "gt_to_pred"))}
            run["cells"][f"{mult:g}"] = row
            del fused
        del vol, mesh, bare
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write(f"tools/bench_mesh_simplify.py --cells {args.cells} --spacings {args.spacings} --cameras {args.cameras} --scale {args.scale} "
                    f"--repeats {args.repeats} --composed-repeats {args.composed_repeats} --samples {args.samples}\n")
            f.write(line + "\n")


if __name__ == "__main__":
    main()
