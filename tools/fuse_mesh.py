#!/usr/bin/env python3
"""ONE mesh of a tiled scene from what its cameras saw: depth maps rendered at the capture's cameras, fused into a truncated signed
distance volume, the zero set written as a PLY.

    python tools/fuse_mesh.py TILEDIR [TILEDIR ...] --cameras camera.log --out FILE.ply [--cells-per-axis 256]
                              [--box X Y Z SX SY SZ] [--trunc T] [--min-weight N] [--scale S] [--max-transparency A]
                              [--views-per-batch B] [--min-faces N] [--min-extent CELLS] [--keep-largest K] [--gpu 0]
                              [--colors diffuse|rgb] [--normals] [--simplify CELL]
                              [--compare GT.ply --threshold T [T ...] [--samples N] [--max-dist D] [--log2dim L] [--seed S]
                               [--normal-consistency]]
                              [--render-score]

Every TILEDIR holds feature.npz and decoder.pth as renderer.export_tile writes and renderer.load_tile reads them.  Each camera of
camera.log (formats.read_campara) is rendered at 1 / --scale of its size; a pixel whose ray kept more than --max-transparency of its
transmittance has no depth.  The maps are fused --views-per-batch at a time over --box (default: the bounding box of the tiles' render
boxes) with --cells-per-axis cells along its longest side; --trunc: the truncation distance in world units (default: 4 x the largest
lattice spacing); a lattice point counts as observed after --min-weight observations.  No level to pick: the surface is the volume's
zero set, in world units; what no ray stopped at never enters it.  Faces that touch a cell with an unobserved corner are dropped
(fusion.support_cull), then --min-faces / --min-extent / --keep-largest drop components (meshing.filter_mesh).
--colors fuses the renders' images with the same weights and writes them as uchar red / green / blue per vertex:
`diffuse` the view-independent part, `rgb` diffuse + specular, each clamped to [0, 1]; a vertex no camera coloured is mid grey.
--normals writes nx / ny / nz per vertex: the volume's own gradient at the vertex, pointing out of the surface;
with --colors one PLY holds both.
--simplify CELL clusters the finished mesh on the world grid of cubic cells of side CELL (world units) as the last step, the normals
and colours averaged with the vertices (meshing.simplify_mesh): fuse fine, hand out coarse.
--compare GT.ply prints the geometric score against GT.ply as the one JSON line of tools/compare_meshes.py.
--render-score prints the image-space score as one JSON line: the finished mesh rendered at the same cameras, with the
fused colours under --colors, against the renders it was fused from (evaluation.compare_renders); the scene is not rendered again.
tools/extract_scene_mesh.py cuts the density's level set instead."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tiles", metavar="TILEDIR", nargs="+", help="directories with feature.npz and decoder.pth: the tiles of one scene")
    ap.add_argument("--cameras", required=True, metavar="camera.log", help="the capture's cameras (formats.read_campara)")
    ap.add_argument("--out", required=True, metavar="FILE.ply")
    ap.add_argument("--cells-per-axis", type=int, default=256, help="lattice cells along the world box's longest side")
    ap.add_argument("--box", type=float, nargs=6, default=None, metavar=("X", "Y", "Z", "SX", "SY", "SZ"),
                    help="world box of the lattice: corner and size (default: the bounding box of the tiles' render boxes)")
    ap.add_argument("--trunc", type=float, default=None, help="truncation distance, world units (default: 4 x the largest lattice spacing)")
    ap.add_argument("--min-weight", type=int, default=1, help="observations a lattice point needs to count as observed")
    ap.add_argument("--scale", type=int, default=1, help="render the cameras at 1 / scale of their size")
    ap.add_argument("--max-transparency", type=float, default=0.5, help="a ray that kept more of its transmittance has no depth")
    ap.add_argument("--views-per-batch", type=int, default=8, help="depth maps held at a time")
    ap.add_argument("--min-faces", type=int, default=0, help="drop components with fewer faces (1: exactly the unused vertices)")
    ap.add_argument("--min-extent", type=int, default=0, help="drop components whose box of cells is shorter than this on every axis")
    ap.add_argument("--keep-largest", type=int, default=None, metavar="K", help="keep only the K components with the most faces")
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--colors", choices=("diffuse", "rgb"), default=None,
                    help="also fuse the renders' colours and write them as red / green / blue per vertex")
    ap.add_argument("--normals", action="store_true", help="also write nx / ny / nz per vertex: the volume's gradient normals")
    ap.add_argument("--simplify", type=float, default=None, metavar="CELL",
                    help="last step: cluster the vertices on a world grid of cells of this side (world units)")
    ap.add_argument("--compare", default=None, metavar="GT.ply",
                    help="after writing the PLY, print the geometric score of the mesh against GT.ply as one JSON line (needs --threshold)")
    ap.add_argument("--render-score", action="store_true",
                    help="print the image-space score of the mesh against the renders it was fused from as one JSON line")
    import scanerf_amd  # noqa: F401
    from scanerf_amd import evaluation
    evaluation.add_score_arguments(ap, required=False)
    return ap


def main(argv=None):
    ap = parser()
    args = ap.parse_args(argv)
    if args.compare and not args.threshold:
        ap.error("--compare needs --threshold")
    from scanerf_amd import evaluation, formats, renderer
    rnd = renderer.TileSetRenderer(f"cuda:{args.gpu}", [renderer.load_tile(p) for p in args.tiles])
    box = None if args.box is None else (args.box[:3], args.box[3:])
    report = {}
    cameras = formats.read_campara(args.cameras, return_shape=True)
    mesh = rnd.fuse_mesh(cameras, args.cells_per_axis, box=box, trunc=args.trunc, max_transparency=args.max_transparency, scale=args.scale,
                         views_per_batch=args.views_per_batch, min_weight=args.min_weight, min_faces=args.min_faces,
                         min_extent=args.min_extent, keep_largest=args.keep_largest, report=report, colors=args.colors,
                         normals=args.normals, simplify=args.simplify, score=args.render_score)
    rgb = None
    if args.colors:
        mesh, rgb = mesh
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    formats.write_ply(args.out, mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(), colors=None if rgb is None else rgb.cpu().numpy(),
                      normals=mesh.normals.cpu().numpy() if args.normals else None)
    sup = report["support"]
    print(f"{args.out}: {len(args.tiles)} tiles, {len(cameras[0])} cameras, {mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} faces")
    print(f"{args.out}: support cull: vertices {sup['vertices'][0]} -> {sup['vertices'][1]}, faces {sup['faces'][0]} -> {sup['faces'][1]}")
    print(f"{args.out}: {report['components']} components, {report['kept_components']} kept; vertices {report['vertices'][0]} -> "
          f"{report['vertices'][1]}, faces {report['faces'][0]} -> {report['faces'][1]}")
    if args.colors:
        print(f"{args.out}: colours ({args.colors}): {report['color']} of {mesh.vertices.shape[0]} vertices uncoloured")
    if args.normals:
        print(f"{args.out}: normals: {report['normals']} of {mesh.vertices.shape[0]} vertices with a zero normal")
    if args.simplify is not None:
        simp = report["simplify"]
        print(f"{args.out}: simplified at cell {args.simplify:g}: vertices {simp['vertices'][0]} -> {simp['vertices'][1]}, faces "
              f"{simp['faces'][0]} -> {simp['faces'][1]}")
    if args.render_score:
        print(evaluation.render_score_line(report["render_score"]))
    if args.compare:
        print(evaluation.score_line((mesh.vertices, mesh.faces), args.compare, args, mesh.vertices.device))
    return 0


if __name__ == "__main__":
    sys.exit(main())
