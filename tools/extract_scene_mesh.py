#!/usr/bin/env python3
"""ONE mesh of a tiled scene: the level set of the tiles' blended density, written as a PLY.

    python tools/extract_scene_mesh.py TILEDIR [TILEDIR ...] --level SIGMA [--cells-per-axis 256]
                                       [--box X Y Z SX SY SZ] --out FILE.ply [--normals] [--route fused|dense] [--gpu 0]
                                       [--min-faces N] [--min-extent CELLS] [--keep-largest K]
                                       [--cameras camera.log --min-views N [--view-bias B] [--view-far D]] [--simplify CELL]
                                       [--colors diffuse|rgb [--color-scale S]]
                                       [--compare GT.ply --threshold T [T ...] [--samples N] [--max-dist D] [--log2dim L] [--seed S]
                                        [--normal-consistency]]

Every TILEDIR holds feature.npz and decoder.pth as renderer.export_tile writes and renderer.load_tile reads them; together they are
the scene renderer.TileSetRenderer draws.  The field is the one it draws: the tiles' densities blended per point with the render-time
xz-distance weights, so the surface runs through the tile faces and margins as the rendered images do, closed there, open only at
the faces of the world box.  The lattice covers --box (corner and size in world units; default: the bounding box of the tiles' render
boxes) with --cells-per-axis cells along its longest side.  --normals stores the vertex normals (nx ny nz): the blended density's own
gradient, weight terms included.  --min-faces / --min-extent / --keep-largest drop floaters and unused vertices by
connected component before the normals are evaluated (meshing.filter_mesh); the component count and the rows before
and after are printed either way.  --cameras camera.log --min-views N first drops the faces none of whose vertices N of the log's
cameras see (the mesh itself occluding; meshing.cull_unseen; --view-bias: half a lattice spacing by default,
--view-far: the cameras' range).  --simplify CELL clusters the finished mesh on the world grid of cubic cells of side CELL as the last
step, the normals averaged with the vertices (meshing.simplify_mesh).  --colors diffuse|rgb (needs --cameras) stores
red / green / blue: the scene rendered at the log's cameras (at 1 / --color-scale of their size) and projected onto the FINAL vertices,
the mesh itself occluding (TileSetRenderer.color_mesh).  --compare GT.ply prints, after the PLY is written, the geometric score of the mesh against GT.ply
(e.g. the dataset's scan) as the one JSON line of tools/compare_meshes.py.  tools/extract_mesh.py writes one open mesh per tile instead."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tiles", metavar="TILEDIR", nargs="+", help="directories with feature.npz and decoder.pth: the tiles of one scene")
    ap.add_argument("--level", type=float, required=True, help="density of the level set (sigma units, > 0)")
    ap.add_argument("--cells-per-axis", type=int, default=256, help="lattice cells along the world box's longest side")
    ap.add_argument("--box", type=float, nargs=6, default=None, metavar=("X", "Y", "Z", "SX", "SY", "SZ"),
                    help="world box of the lattice: corner and size (default: the bounding box of the tiles' render boxes)")
    ap.add_argument("--out", required=True, metavar="FILE.ply")
    ap.add_argument("--normals", action="store_true", help="store vertex normals (nx ny nz): the blended density's gradient")
    ap.add_argument("--route", choices=("fused", "dense"), default="fused", help="dense: the composed route (small lattices only)")
    ap.add_argument("--min-faces", type=int, default=0, help="drop components with fewer faces (1: exactly the unused vertices)")
    ap.add_argument("--min-extent", type=int, default=0, help="drop components whose box of cells is shorter than this on every axis")
    ap.add_argument("--keep-largest", type=int, default=None, metavar="K", help="keep only the K components with the most faces")
    ap.add_argument("--cameras", default=None, metavar="camera.log", help="the capture's cameras (formats.read_campara): cull what they do not see")
    ap.add_argument("--min-views", type=int, default=0, metavar="N", help="keep a face iff N cameras see one of its vertices (needs --cameras)")
    ap.add_argument("--view-bias", type=float, default=None, metavar="B", help="start of a sight line, off the vertex (default: half a lattice spacing)")
    ap.add_argument("--view-far", type=float, default=None, metavar="D", help="the cameras' range (default: no limit)")
    ap.add_argument("--simplify", type=float, default=None, metavar="CELL",
                    help="last step: cluster the vertices on a world grid of cells of this side (world units)")
    ap.add_argument("--colors", choices=("diffuse", "rgb"), default=None,
                    help="store vertex colours: the scene's renders at --cameras projected onto the final vertices")
    ap.add_argument("--color-scale", type=int, default=1, metavar="S", help="render the cameras at 1 / S of their size for --colors")
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--compare", default=None, metavar="GT.ply",
                    help="after writing the PLY, print the geometric score of the mesh against GT.ply as one JSON line (needs --threshold)")
    import scanerf_amd  # noqa: F401
    from scanerf_amd import evaluation
    evaluation.add_score_arguments(ap, required=False)
    return ap


def main(argv=None):
    ap = parser()
    args = ap.parse_args(argv)
    if args.compare and not args.threshold:
        ap.error("--compare needs --threshold")
    if args.min_views > 0 and not args.cameras:
        ap.error("--min-views needs --cameras")
    if args.colors and not args.cameras:
        ap.error("--colors needs --cameras")
    from scanerf_amd import evaluation, formats, renderer
    rnd = renderer.TileSetRenderer(f"cuda:{args.gpu}", [renderer.load_tile(p) for p in args.tiles])
    box = None if args.box is None else (args.box[:3], args.box[3:])
    report = {}
    cameras = formats.read_campara(args.cameras, return_shape=True) if args.cameras else None
    mesh = rnd.extract_mesh(args.level, args.cells_per_axis, box=box, route=args.route, normals=args.normals, min_faces=args.min_faces,
                            min_extent=args.min_extent, keep_largest=args.keep_largest, report=report, cameras=cameras,
                            min_views=args.min_views, view_bias=args.view_bias, view_far=args.view_far, simplify=args.simplify,
                            **(dict(colors=args.colors, color_scale=args.color_scale) if args.colors else {}))
    rgb = None
    if args.colors:
        mesh, rgb = mesh
    out_dir = os.path.dirname(os.path.abspath(args.out))
    os.makedirs(out_dir, exist_ok=True)
    formats.write_ply(args.out, mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(),
                      normals=mesh.normals.cpu().numpy() if args.normals else None,
                      colors=None if rgb is None else rgb.clamp(0.0, 1.0).cpu().numpy())
    print(f"{args.out}: {len(args.tiles)} tiles, {mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} faces")
    print(f"{args.out}: {report['components']} components, {report['kept_components']} kept; vertices {report['vertices'][0]} -> "
          f"{report['vertices'][1]}, faces {report['faces'][0]} -> {report['faces'][1]}")
    if "cull" in report:
        cull, hist = report["cull"], report["cull"]["views_histogram"]
        print(f"{args.out}: unseen parts culled first: vertices {cull['vertices'][0]} -> {cull['vertices'][1]}, faces {cull['faces'][0]} -> "
              f"{cull['faces'][1]}; {hist[0] if hist else 0} vertices seen by no camera, at most {max(len(hist) - 1, 0)} views")
    if args.simplify is not None:
        simp = report["simplify"]
        print(f"{args.out}: simplified at cell {args.simplify:g}: vertices {simp['vertices'][0]} -> {simp['vertices'][1]}, faces "
              f"{simp['faces'][0]} -> {simp['faces'][1]}")
    if rgb is not None:
        print(f"{args.out}: vertex colours ({args.colors}) from {len(cameras[0])} cameras at 1/{args.color_scale} of their size")
    if args.compare:
        print(evaluation.score_line((mesh.vertices, mesh.faces), args.compare, args, mesh.vertices.device))
    return 0


if __name__ == "__main__":
    sys.exit(main())
