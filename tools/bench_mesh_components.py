"""Cost of the mesh components and the filter by component (csrc/mesh_components.hip; meshing.mesh_components / filter_mesh;
DESIGN.md 4.17) on the scene meshes tools/bench_scene_mesh.py extracts, at its two lattice sizes:

  * `fused`      labelling (scanerf_mesh_components_label and the host read of C), the table (scanerf_mesh_components_table) and the
                 filter with keep_largest=1 (scanerf_mesh_filter_count, the host read of (V', F'), the outputs, scanerf_mesh_filter_emit),
                 timed separately, and meshing.filter_mesh as a whole;
  * `composed`   the same three steps in torch ops (meshing's route="composed": label propagation with a host read per round,
                 bincount / scatter_reduce, boolean indexing and cumsum) -- not the code under test;
  * `extract`    the extraction of the same mesh (TileSetRenderer.extract_mesh, unchanged code), beside them.

    python tools/bench_mesh_components.py [--cells 256,512] [--log2-T 19] [--repeats 7] [--out profiles/mesh_components_bench.json]

Host clock around work that ends in a device synchronise; every shape is run once before it is timed; the routes alternate `repeats`
times and every run is reported, with medians, spreads (max - min over the median) and the ratios fused / composed and filter /
extraction.  Beside the labelling: the face list's bytes over its time, and the time HBM would take to stream those bytes at the
measured copy rate.  Both routes' results are compared bit for bit before anything is timed.  Writes one JSON document, rewritten
after every lattice."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_COPY_RATE = 6.29e12     # bytes / s: the float4 copy rate measured on an MI355X (8.0e12 is the specification's peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="256,512", help="lattice cells along the scene box's longest side, one mesh each")
    ap.add_argument("--log2-T", type=int, default=19)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_components_bench.json"))
    args = ap.parse_args()
    import scanerf_amd  # noqa
    from bench_scene_mesh import build_scene, clock
    from scanerf_amd import _capi, meshing, render
    dev = "cuda:0"
    lib = _capi.lib()
    rnd = build_scene(dev, args.log2_T)
    x0 = meshing.lattice_positions([32, 32, 32], dev)
    sigma0, _, _ = render.sigma_normals_points(x0, rnd.feature_tables[0], rnd.resolution[0], rnd.params[0], torch.ones(32, device=dev))
    level = float(sigma0.median())                         # tools/bench_scene_mesh.py's level
    out = {"device": torch.cuda.get_device_name(0), "tiles": int(rnd.feature_tables.shape[0]), "log2_T": args.log2_T, "level": level,
           "rule": "keep_largest=1", "hbm_copy_rate_bytes_per_s": HBM_COPY_RATE, "runs": {}}
    i32 = torch.int32

    for cells in (int(s) for s in args.cells.split(",")):
        mesh = rnd.extract_mesh(level, cells)
        V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
        faces, cellsv = mesh.faces, mesh.cells
        nbytes = int(lib.scanerf_mesh_components_scratch_bytes(V, F))
        state = {}

        def fused_label():
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            labels = torch.empty(V, dtype=i32, device=dev)
            _capi.check(lib.scanerf_mesh_components_label(faces.data_ptr(), V, F, labels.data_ptr(), scratch.data_ptr(), nbytes, _capi.stream()), "label")
            state.update(scratch=scratch, labels=labels, C=int(scratch[:8].view(torch.int64).item()))

        def fused_table():
            C = state["C"]
            rows = [torch.empty(s, dtype=i32, device=dev) for s in ((C,), (C,), (C,), (C, 3), (C, 3))]
            _capi.check(lib.scanerf_mesh_components_table(faces.data_ptr(), cellsv.data_ptr(), state["labels"].data_ptr(), V, F,
                                                          state["scratch"].data_ptr(), nbytes, C, *(t.data_ptr() for t in rows), _capi.stream()), "table")
            state["rows"] = rows

        def fused_filter():
            C, scratch = state["C"], state["scratch"]
            head = (faces.data_ptr(), state["labels"].data_ptr(), state["keep"].data_ptr(), V, F, C, scratch.data_ptr(), nbytes)
            _capi.check(lib.scanerf_mesh_filter_count(*head, _capi.stream()), "count")
            Vk, Fk = scratch[8:24].view(torch.int64).tolist()
            o = [torch.empty((Vk, 3), dtype=torch.float32, device=dev), torch.empty((Fk, 3), dtype=i32, device=dev),
                 torch.empty((Vk, 3), dtype=i32, device=dev), torch.empty((Vk, 3), dtype=torch.float32, device=dev)]
            _capi.check(lib.scanerf_mesh_filter_emit(*head, mesh.vertices.data_ptr(), cellsv.data_ptr(), mesh.lattice.data_ptr(), None,
                                                     o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), None, Vk, Fk,
                                                     _capi.stream()), "emit")
            state["kept"] = (Vk, Fk)

        def composed_label():
            state["lab"] = meshing._labels_composed(faces, V)

        def composed_table():
            state["crows"] = meshing._table_composed(faces, cellsv, state["lab"])

        # warm every shape, and compare the routes bit for bit before timing anything
        a = meshing.mesh_components(faces, V, cellsv)
        b = meshing.mesh_components(faces, V, cellsv, route="composed")
        assert all(torch.equal(x, y) for x, y in zip(a, b)), "the fused and the composed components differ"
        fa = meshing.filter_mesh(mesh, keep_largest=1)
        fb = meshing.filter_mesh(mesh, keep_largest=1, route="composed")
        assert all(torch.equal(x, y) for x, y in zip(fa[:4], fb[:4])), "the fused and the composed filtered meshes differ"
        fused_label(), fused_table()
        rows = state["rows"]
        order = torch.argsort(((2 ** 31 - 1 - rows[2].to(torch.int64)) << 32) | rows[0].to(torch.int64))
        keep = torch.zeros(state["C"], dtype=torch.uint8, device=dev)
        keep[order[0]] = 1
        state["keep"] = keep
        fused_filter(), composed_label(), composed_table()
        del a, b, fa, fb

        steps = {"extract_ms": lambda: rnd.extract_mesh(level, cells),
                 "fused_label_ms": fused_label, "fused_table_ms": fused_table, "fused_filter_ms": fused_filter,
                 "fused_filter_mesh_ms": lambda: meshing.filter_mesh(mesh, keep_largest=1),
                 "composed_label_ms": composed_label, "composed_table_ms": composed_table,
                 "composed_filter_mesh_ms": lambda: meshing.filter_mesh(mesh, keep_largest=1, route="composed")}
        runs = [{k: clock(fn)[0] for k, fn in steps.items()} for _ in range(args.repeats)]      # the steps alternate within a repeat
        med = {k: statistics.median(r[k] for r in runs) for k in steps}
        face_bytes = 12 * F
        row = {"V": V, "F": F, "components": state["C"], "kept": {"V": state["kept"][0], "F": state["kept"][1]}, "scratch_bytes": nbytes,
               "alternating": runs, "median_ms": med,
               "spread": {k: (max(r[k] for r in runs) - min(r[k] for r in runs)) / med[k] for k in steps},
               "fused_over_composed": {k: med[f"fused_{k}_ms"] / med[f"composed_{k}_ms"] for k in ("label", "table", "filter_mesh")},
               "filter_mesh_over_extract": med["fused_filter_mesh_ms"] / med["extract_ms"],
               "face_list_bytes": face_bytes, "face_list_bytes_per_s_in_labelling": face_bytes / (med["fused_label_ms"] * 1e-3),
               "face_list_hbm_stream_ms": face_bytes / HBM_COPY_RATE * 1e3}
        out["runs"][str(cells)] = row
        json.dump(out, open(args.out, "w"), indent=1)
        del mesh, faces, cellsv
        state.clear()
    print(json.dumps({c: {k: r[k] for k in ("V", "F", "components", "median_ms", "spread", "fused_over_composed", "filter_mesh_over_extract",
                                            "face_list_bytes_per_s_in_labelling", "face_list_hbm_stream_ms")} for c, r in out["runs"].items()}))


if __name__ == "__main__":
    main()
