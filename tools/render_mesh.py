#!/usr/bin/env python3
"""Render a mesh, with the vertex normals and colours its PLY holds, at a set of cameras.

    python tools/render_mesh.py MESH.ply --cameras camera.log --out DIR [--scale S] [--log2dim L] [--views-per-batch B] [--gpu 0]

Each camera of camera.log (formats.read_campara) is rendered at 1 / --scale of its size (K scaled as fusion.scale_cameras does) by
evaluation.render_mesh, --views-per-batch at a time.  DIR/view_00000.npz, ... hold per view: depth [H,W] f32 (z-depth, 0 = nothing),
face [H,W] i32 (-1 = nothing), normal [H,W,3] f32 (the interpolated nx / ny / nz of the PLY, or the face normals where it has none)
and, where the PLY holds red / green / blue, color [H,W,3] f32 in 0..1.  Image formats are out of scope: the arrays are the output."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mesh", metavar="MESH.ply")
    ap.add_argument("--cameras", required=True, metavar="camera.log", help="the cameras (formats.read_campara)")
    ap.add_argument("--out", required=True, metavar="DIR", help="receives one view_NNNNN.npz per camera")
    ap.add_argument("--scale", type=int, default=1, help="render the cameras at 1 / scale of their size")
    ap.add_argument("--log2dim", type=int, default=6, help="grid cells per axis of the tracer, as a power of two (4..7)")
    ap.add_argument("--views-per-batch", type=int, default=8, help="views rendered per launch")
    ap.add_argument("--gpu", type=int, default=0)
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    import numpy as np
    import torch

    import scanerf_amd  # noqa: F401
    from scanerf_amd import evaluation, formats, fusion
    props = formats.ply_vertex_properties(args.mesh)
    has_n, has_c = all(p in props for p in ("nx", "ny", "nz")), all(p in props for p in ("red", "green", "blue"))
    arrays = list(formats.read_ply(args.mesh, normals=has_n, colors=has_c))
    vertices, faces = arrays[0], arrays[1]
    normals = torch.from_numpy(arrays[2]) if has_n else True
    colors = torch.from_numpy(arrays[-1].astype(np.float32) / np.float32(255.0)) if has_c else None
    ks, c2ws, H, W = formats.read_campara(args.cameras, return_shape=True)
    scale = fusion._positive_int(args.scale, "scale")
    h, w = int(H) // scale, int(W) // scale
    if h < 1 or w < 1:
        raise SystemExit(f"render_mesh: H={H} W={W} leave no pixel at scale={scale}")
    device = torch.device("cuda", args.gpu)
    os.makedirs(args.out, exist_ok=True)
    n = 0
    for first, batch in evaluation.render_mesh((vertices, faces), (fusion.scale_cameras(ks, scale), c2ws, h, w), colors=colors,
                                               normals=normals, log2dim=args.log2dim, views_per_batch=args.views_per_batch,
                                               device=device):
        host = {k: v.cpu().numpy() for k, v in batch.items()}
        for b in range(host["depth"].shape[0]):
            np.savez(os.path.join(args.out, f"view_{first + b:05d}.npz"), **{k: v[b] for k, v in host.items()})
            n += 1
    print(f"{args.out}: {n} views of {h} x {w}, {vertices.shape[0]} vertices, {faces.shape[0]} faces"
          f"{', normals' if has_n else ', face normals'}{', colours' if has_c else ''}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
