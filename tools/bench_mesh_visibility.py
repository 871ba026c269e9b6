"""Cost of the point-visibility op: the fused kernel (FastMesh.point_views, csrc/mesh_visibility.hip) beside the same
answer composed from the ops that existed before it -- per camera the frustum test as torch elementwise ops, FastMesh.first_hit on the
pairs in view, a comparison and a sum (FastMesh.point_views(route="composed")).

    python tools/bench_mesh_visibility.py [--repeat 10] [--warmup 2] [--mesh-n 500] [--cameras 64] [--out profiles/mesh_visibility_bench.txt]

Scene: the procedural terrain of tools/bench_tile_alloc.py (2 * mesh_n^2 faces, default 500 000, over [-10,10]^2), its vertices as the
points, `cameras` 1920 x 1080 cameras on that tool's ring, bias = half the mean edge.  Each figure is the median of `repeat` runs over
ALL cameras after `warmup`, timed with device events, both routes in this one process.  Also reported: pairs per second, the share of
the pairs in view, the walked pairs per second, the occupied cells and ray / triangle tests per walked pair (the counted entry), the
kernel's registers / LDS / scratch (read from the library's code object when llvm-readelf is at hand), and whether the two routes give
the same bits.  Not measured: other camera counts, log2dim 7, real captures."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LLVM = "/opt/rocm/lib/llvm/bin"


def kernel_resources(lib_path, needle="k_point_viewsILb1ELb0"):
    """VGPRs / SGPRs / LDS bytes / scratch bytes / spills of the product kernel (pre-gathered triangles, no counters), or None."""
    try:
        with tempfile.TemporaryDirectory() as tmp:
            dst = os.path.join(tmp, "lib.so")
            with open(lib_path, "rb") as f, open(dst, "wb") as g:
                g.write(f.read())
            subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", dst], check=True, capture_output=True)
            for co in sorted(f for f in os.listdir(tmp) if "gfx950" in f):
                notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", os.path.join(tmp, co)], check=True, capture_output=True, text=True).stdout
                for blk in notes.split("- .agpr_count:")[1:]:
                    if needle in blk:
                        get = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
                        return {"vgprs": get("vgpr_count"), "sgprs": get("sgpr_count"), "lds_bytes": get("group_segment_fixed_size"),
                                "scratch_bytes": get("private_segment_fixed_size"), "spills": get("vgpr_spill_count")}
    except (OSError, subprocess.SubprocessError, AttributeError):
        pass
    return None


def counted(fm, pts, ks, c2ws, H, W, bias):
    """-> (views, [pairs walked, occupied cells looked at, ray / triangle tests]) from the counted entry."""
    from scanerf_amd import _capi
    from scanerf_amd.allocation import _cameras
    k9, c12 = _cameras(ks, c2ws, pts.device)
    views = torch.empty(pts.shape[0], dtype=torch.int32, device=pts.device)
    counters = torch.zeros(3, dtype=torch.int64, device=pts.device)
    p = lambda t: None if t is None else t.data_ptr()
    _capi.check(_capi.tool("scanerf_mesh_point_views_counted")(
        p(pts), pts.shape[0], p(k9), p(c12), k9.shape[0], H, W, bias, 0.0, float("inf"), p(fm.vertices), p(fm.faces), p(fm.tris),
        p(fm.bitmask), p(fm.rank), p(fm.start_num), p(fm.cell_faces), p(fm.scene_info), fm.log2dim, p(views), None, p(counters),
        _capi.stream()), "mesh_point_views_counted")
    return views, counters.tolist()


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
    from scanerf_amd import _capi
    from scanerf_amd.fastmesh import FastMesh
    dev = "cuda:0"
    H, W = 1080, 1920
    V, F = height_field(args.mesh_n, dev)
    fm = FastMesh.from_arrays(V, F, dev)
    ks, c2ws = [], []
    for c in range(args.cameras):
        a = 2 * np.pi * c / args.cameras
        c2w, K = FR.look_at((8.5 * np.cos(a), 8.5 * np.sin(a), 3.0 + 0.02 * c), (3 * np.cos(a + 2.5), 3 * np.sin(a + 2.5), 0.0), H, W, 1400.0)
        ks.append(K)
        c2ws.append(c2w)
    ks, c2ws = torch.from_numpy(np.stack(ks)).to(dev), torch.from_numpy(np.stack(c2ws)).to(dev)
    pts = fm.vertices
    tri = fm.vertices[fm.faces.long()]
    edges = torch.cat([(tri[:, 1] - tri[:, 0]).norm(dim=1), (tri[:, 2] - tri[:, 1]).norm(dim=1), (tri[:, 0] - tri[:, 2]).norm(dim=1)])
    bias = 0.5 * float(edges.mean())
    fused = lambda: fm.point_views(pts, ks, c2ws, H, W, bias, want_mask=True)
    composed = lambda: fm.point_views(pts, ks, c2ws, H, W, bias, want_mask=True, route="composed")
    (av, am), (bv, bm) = fused(), composed()
    cv, (walked, cells, tests) = counted(fm, pts, ks, c2ws, H, W, bias)
    pairs = int(pts.shape[0]) * args.cameras
    res = {"device": torch.cuda.get_device_name(0), "faces": int(F.shape[0]), "points": int(pts.shape[0]), "cameras": args.cameras,
           "frame": [H, W], "log2dim": fm.log2dim, "pregathered": fm.tris is not None, "bias": round(bias, 5), "repeat": args.repeat,
           "cameras_per_pass": int(_capi.tool("scanerf_mesh_point_views_cameras_per_pass")()),
           "fused_ms": round(event_ms(fused, args.repeat, args.warmup), 3),
           "composed_ms": round(event_ms(composed, args.repeat, args.warmup), 3),
           "pairs": pairs, "pairs_in_view": walked, "share_in_view": round(walked / pairs, 4),
           "pairs_seen": int(av.sum()), "points_seen_by_no_camera": int((av == 0).sum()),
           "cells_per_walked_pair": round(cells / max(walked, 1), 2), "tests_per_walked_pair": round(tests / max(walked, 1), 2),
           "views_that_differ": int((av != bv).sum()), "mask_words_that_differ": int((am != bm).sum()),
           "counted_entry_agrees": bool(torch.equal(cv, av)), "kernel": kernel_resources(_capi.LIB_PATH)}
    res["pairs_per_s"] = round(pairs / res["fused_ms"] * 1e3)
    res["walked_pairs_per_s"] = round(walked / res["fused_ms"] * 1e3)
    res["speedup"] = round(res["composed_ms"] / res["fused_ms"], 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"tools/bench_mesh_visibility.py --repeat {args.repeat} --warmup {args.warmup} --mesh-n {args.mesh_n} --cameras {args.cameras}\n")
            f.write(line + "\n")


if __name__ == "__main__":
    main()
