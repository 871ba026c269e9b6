#!/usr/bin/env python3
"""Tile allocation from mesh depth: the reference's preprocess/build_tiles.py as a command.

    python tools/build_tiles.py DATADIR --tile-size X Y Z [--overlap-ratio 0.2] [--offset X Y Z] [--expect-num N]
                                [--min-num-image N] [--max-dim-tile X Y Z] [--scene-type outdoor|indoor] [--scale 4] [--gpu 0]

Reads DATADIR/mesh/mesh.ply, DATADIR/camera.log and, when present, DATADIR/ignore.log (camera ids to leave out: one id, or `first
last` for first .. last - 1, per line); writes DATADIR/tiles/tile_info.txt and DATADIR/tiles/training_views.txt, the two files
every training entry point starts from.  The options are the ALLOCATION keys of the reference's scene file (TILE_SIZE,
OVERLAP_RATIO, OFFSET, EXPECT_NUM, MIN_NUM_IMAGE, MAX_DIM_TILE, SCENE_TYPE)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("datadir", metavar="DATADIR")
    ap.add_argument("--tile-size", type=float, nargs=3, required=True, metavar=("X", "Y", "Z"), help="side lengths of a tile")
    ap.add_argument("--overlap-ratio", type=float, default=0.2, help="share of a tile's side its neighbour overlaps")
    ap.add_argument("--offset", type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("X", "Y", "Z"),
                    help="moves the grid's origin off the mesh's minimum corner")
    ap.add_argument("--expect-num", type=int, required=True, help="number of tiles wanted")
    ap.add_argument("--min-num-image", type=int, default=60, help="a tile needs strictly more views than this")
    ap.add_argument("--max-dim-tile", type=int, nargs=3, default=[100000, 100000, 100000], metavar=("X", "Y", "Z"),
                    help="most tiles per axis")
    ap.add_argument("--scene-type", choices=("outdoor", "indoor"), default="outdoor")
    ap.add_argument("--scale", type=int, default=4, help="coverage is counted on the frame reduced by this factor")
    ap.add_argument("--gpu", type=int, default=0)
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    import torch

    import scanerf_amd  # noqa: F401
    from scanerf_amd import allocation, formats
    ks, c2ws, H, W = formats.read_campara(os.path.join(args.datadir, "camera.log"), True)
    ignore = allocation.read_ignore_log(os.path.join(args.datadir, "ignore.log"))
    result = allocation.allocate_tiles(os.path.join(args.datadir, "mesh", "mesh.ply"), ks, c2ws, H, W, tile_size=args.tile_size,
                                       overlap_ratio=args.overlap_ratio, offset=args.offset, expect_num=args.expect_num,
                                       min_num_image=args.min_num_image, max_dim_tile=args.max_dim_tile, scene_type=args.scene_type,
                                       ignore=ignore, scale=args.scale, device=torch.device("cuda", args.gpu))
    tile_dir = os.path.join(args.datadir, "tiles")
    allocation.write_allocation(tile_dir, result)
    print(f"{len(result['all_corners'])} candidate tiles, {len(ks)} cameras ({len(ignore)} ignored) -> {len(result['tiles'])} tiles "
          f"with {[len(v) for v in result['views']]} views in {tile_dir}")


if __name__ == "__main__":
    main()
