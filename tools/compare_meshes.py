#!/usr/bin/env python3
"""Geometric score of one mesh against another: accuracy, completeness, chamfer, precision / recall / F-score.

    python tools/compare_meshes.py PRED.ply GT.ply --samples N --threshold T [T ...] [--max-dist D] [--log2dim L] [--seed S]
                                   [--normal-consistency] [--json FILE] [--distances FILE.npz] [--gpu G]

N points are drawn on each surface (area-weighted, stratified) and each is asked the exact distance to the other mesh
(evaluation.compare_meshes; the query is csrc/mesh_distance.hip).  The result is printed as ONE JSON line: per direction (pred_to_gt
= accuracy, gt_to_pred = completeness) mean / median / rms over the points found and the share not found within --max-dist; per
threshold precision, recall and fscore; chamfer = the mean of the two means.  --normal-consistency adds the orientation score
(DESIGN.md 4.22): per direction the mean and mean absolute dot product of the sampled face's and the nearest face's unit normals, and
the share of samples skipped (not found, or a face without area).  --json also stores the line; --distances stores the
sample points, their faces, the distances and the nearest faces of both directions."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parser():
    import scanerf_amd  # noqa: F401
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("pred", metavar="PRED.ply")
    ap.add_argument("gt", metavar="GT.ply")
    from scanerf_amd import evaluation
    evaluation.add_score_arguments(ap, required=True)
    ap.add_argument("--json", default=None, metavar="FILE", help="also write the line here")
    ap.add_argument("--distances", default=None, metavar="FILE.npz", help="store sample points, distances and faces of both directions")
    ap.add_argument("--gpu", type=int, default=0)
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    from scanerf_amd import evaluation
    line = evaluation.score_line(args.pred, args.gt, args, f"cuda:{args.gpu}", args.distances)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
