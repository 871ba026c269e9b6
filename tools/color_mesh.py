#!/usr/bin/env python3
"""Colour the vertices of any mesh from posed images: project, sample, blend.

    python tools/color_mesh.py MESH.ply --cameras camera.log --images IMAGES.npy [-o OUT.ply] [--bias B] [--min-cos C] [--far D]
                               [--no-normals] [--views-per-batch B] [--fill R G B] [--log2dim L] [--gpu 0]

IMAGES.npy holds one image per camera of camera.log (formats.read_campara), [C,H,W,3], uint8 (0..255) or float32 (0..1); it is opened
memory-mapped and moved to the GPU --views-per-batch images at a time.  Image file formats are out of scope: the array is the input.
Every vertex is projected into every camera; the cameras that see it (the mesh itself occluding, a sight line starting --bias towards
the eye: half the mean edge length by default) are sampled bilinearly and blended, weighted by the cosine between the vertex normal
(the PLY's nx / ny / nz, unless --no-normals) and the direction to the eye; --min-cos drops grazing views.  A vertex no camera
contributed to gets --fill.  OUT.ply (default: MESH.colored.ply) is the input mesh with red / green / blue."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mesh", metavar="MESH.ply")
    ap.add_argument("--cameras", required=True, metavar="camera.log", help="the cameras (formats.read_campara)")
    ap.add_argument("--images", required=True, metavar="IMAGES.npy", help="[C,H,W,3] uint8 or float32, one image per camera")
    ap.add_argument("-o", "--out", default=None, metavar="OUT.ply", help="default: MESH.colored.ply")
    ap.add_argument("--bias", type=float, default=None, metavar="B", help="start of a sight line, off the vertex (default: half the mean edge)")
    ap.add_argument("--min-cos", type=float, default=0.0, metavar="C", help="drop views whose cosine to the vertex normal is not above C, in [0, 1)")
    ap.add_argument("--far", type=float, default=float("inf"), metavar="D", help="the cameras' range (default: no limit)")
    ap.add_argument("--no-normals", action="store_true", help="equal weights, also where the PLY holds normals")
    ap.add_argument("--views-per-batch", type=int, default=8, help="images held on the GPU at a time")
    ap.add_argument("--fill", type=float, nargs=3, default=(0.5, 0.5, 0.5), metavar=("R", "G", "B"), help="colour of a vertex nobody saw")
    ap.add_argument("--log2dim", type=int, default=6, help="grid cells per axis of the tracer, as a power of two (4..7)")
    ap.add_argument("--gpu", type=int, default=0)
    return ap


def main(argv=None):
    ap = parser()
    args = ap.parse_args(argv)
    if not 0.0 <= args.min_cos < 1.0:
        ap.error("--min-cos must lie in [0, 1)")
    if args.views_per_batch < 1:
        ap.error("--views-per-batch must be positive")
    import numpy as np
    import torch

    import scanerf_amd  # noqa: F401
    from scanerf_amd import formats, meshing
    props = formats.ply_vertex_properties(args.mesh)
    has_n = all(p in props for p in ("nx", "ny", "nz"))
    arrays = formats.read_ply(args.mesh, normals=has_n)
    ks, c2ws, H, W = formats.read_campara(args.cameras, return_shape=True)
    images = np.load(args.images, mmap_mode="r")
    if images.ndim != 4 or images.shape[0] != len(ks) or images.shape[3] != 3 or images.dtype not in (np.uint8, np.float32):
        raise SystemExit(f"color_mesh: {args.images} must be [C,H,W,3] uint8 or float32 with C={len(ks)}, got {images.shape} {images.dtype}")
    if tuple(images.shape[1:3]) != (int(H), int(W)):
        raise SystemExit(f"color_mesh: the images are {images.shape[1]} x {images.shape[2]}, the cameras {int(H)} x {int(W)}")
    device = torch.device("cuda", args.gpu)
    normals = torch.from_numpy(arrays[2]).to(device) if has_n else None
    mesh = meshing.Mesh(torch.from_numpy(arrays[0]).to(device), torch.from_numpy(arrays[1]).to(device), None, None, normals)
    bias = meshing.default_edge_bias(mesh) if args.bias is None else args.bias
    report = {}
    colors, valid = meshing.color_from_views(mesh, images, ks, c2ws, bias, normals=None if args.no_normals else "mesh", far=args.far,
                                             min_cos=args.min_cos, views_per_batch=args.views_per_batch, fill=args.fill,
                                             log2dim=args.log2dim, report=report)
    out = args.out or os.path.splitext(args.mesh)[0] + ".colored.ply"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    formats.write_ply(out, arrays[0], arrays[1], normals=arrays[2] if has_n else None, colors=colors.clamp(0.0, 1.0).cpu().numpy())
    hist = report["count_histogram"]
    print(f"{out}: {arrays[0].shape[0]} vertices coloured from {len(ks)} images of {int(H)} x {int(W)} (bias {bias:g}"
          f"{', cosine weights' if has_n and not args.no_normals else ', equal weights'}); {report['invalid']} vertices got the fill colour, "
          f"at most {max(len(hist) - 1, 0)} views per vertex")
    return 0


if __name__ == "__main__":
    sys.exit(main())
