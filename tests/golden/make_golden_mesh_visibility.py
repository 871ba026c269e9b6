"""Writes tests/golden/g23_mesh_visibility.npz: the float64 brute-force reference of the point-visibility op
(tests/mesh_visibility_reference.py) for its large cases (the terrain at both biases, the many-cameras ring), as packed bits with a digest of
the inputs.  numpy only; ~35 s.  Run from the repository root: python tests/golden/make_golden_mesh_visibility.py"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import mesh_visibility_reference as MV  # noqa: E402

if __name__ == "__main__":
    MV.write_golden()
    for case in (MV.terrain(), MV.many_cameras(), MV.terrain(MV.SMALL_BIAS)):
        print(case["name"], MV.census(case))
