#!/usr/bin/env python3
"""Simplify a PLY mesh by vertex clustering: the vertices in one cell of a world grid become one vertex.

    python tools/simplify_mesh.py IN.ply OUT.ply --cell H [--origin X Y Z] [--gpu 0]

The grid has cubic cells of side --cell (world units) and a corner at --origin (default 0 0 0): two meshes simplified separately
with the same --cell and --origin cluster alike.  A cluster's vertex is the mean of its members; the normals (nx / ny / nz) and the
colours (uchar red / green / blue) IN.ply holds are averaged with them and written to OUT.ply, the normals renormalised.  Faces are
re-indexed, those that lose a corner disappear, the rest keep their order and winding; duplicate faces are kept.  A --cell below the
vertex spacing returns the input.  (meshing.simplify_mesh; the definition: include/scanerf_mesh_tools_hip.h.)
tools/fuse_mesh.py and tools/extract_scene_mesh.py take --simplify CELL and do this as their last step."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("input", metavar="IN.ply")
    ap.add_argument("output", metavar="OUT.ply")
    ap.add_argument("--cell", type=float, required=True, metavar="H", help="side of the cluster cells, world units")
    ap.add_argument("--origin", type=float, nargs=3, default=(0.0, 0.0, 0.0), metavar=("X", "Y", "Z"), help="a corner of the grid")
    ap.add_argument("--gpu", type=int, default=0)
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    import numpy as np
    import torch

    import scanerf_amd  # noqa: F401
    from scanerf_amd import formats, meshing
    props = formats.ply_vertex_properties(args.input)
    has_normals = all(p in props for p in ("nx", "ny", "nz"))
    has_colors = all(p in props for p in ("red", "green", "blue"))
    arrays = list(formats.read_ply(args.input, normals=has_normals, colors=has_colors))
    vertices, faces = arrays[0], arrays[1]
    normals = arrays[2] if has_normals else None
    colors = arrays[-1].astype(np.float32) / np.float32(255.0) if has_colors else None
    dev = f"cuda:{args.gpu}"
    gpu = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    report = {}
    out = meshing.simplify_mesh(meshing.Mesh(gpu(vertices), gpu(faces), None, None, gpu(normals)), args.cell, origin=tuple(args.origin),
                                colors=gpu(colors), report=report)
    mesh, rgb = out if has_colors else (out, None)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    formats.write_ply(args.output, mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(),
                      normals=mesh.normals.cpu().numpy() if has_normals else None, colors=None if rgb is None else rgb.cpu().numpy())
    print(f"{args.output}: cell {args.cell:g}: vertices {report['vertices'][0]} -> {report['vertices'][1]}, faces {report['faces'][0]} -> "
          f"{report['faces'][1]}; the largest cluster has {report['largest_cluster']} vertices"
          + ("; normals" if has_normals else "") + ("; colours" if has_colors else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
