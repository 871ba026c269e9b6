#!/usr/bin/env python3
"""The judge() lines of `pytest -m gpu -s tests/test_gpu_scene_mesh.py > scene.log` as the markdown table of
profiles/scene_mesh_error.md: every judged case, the kernel's vertex error (lattice steps) beside the float32 yardstick's, their
ratios (the yardstick's figure taken as at least 2^-24, as tests/surface_nets_reference.py forms every bound) and the largest ratios
against the project's K = (8, 16).  K is surface_nets_reference's figure: it is read here, never derived from this run.

    python tools/scene_mesh_error_summary.py scene.log > profiles/scene_mesh_error.md"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

FLOOR = 2.0 ** -24
LINE = re.compile(r"^[.F]*(.+?): op (.+?) \| f32 ref (.+?) \| ratio")


def main(path):
    import scene_mesh_reference as M
    rows, seen = [], set()
    for ln in open(path):
        m = LINE.match(ln.strip())
        if m and m.group(1) not in seen:
            seen.add(m.group(1))
            a, b = ([float(v) for v in m.group(k).split(" / ")] for k in (2, 3))
            rows.append((m.group(1), m.group(2), m.group(3), [x / max(y, FLOOR) for x, y in zip(a, b)]))
    print("# Scene mesh: the fused route against float64 (tests/test_gpu_scene_mesh.py on an MI355X)\n")
    print("Cells and faces are exact outside the ambiguity band in every case (the test asserts it).  Vertices, in lattice steps:\n")
    print("| case and tensor | kernel: median / p99 / max / pooled | float32 yardstick | ratios (yardstick floored at 2^-24) |")
    print("|---|---|---|---|")
    for name, op, ref, r in rows:
        print(f"| {name} | {op} | {ref} | " + " / ".join(f"{v:.2f}" for v in r) + " |")
    q = max((max(r[0], r[1], r[3]), n) for n, _, _, r in rows)
    mx = max((r[2], n) for n, _, _, r in rows)
    print(f"\nlargest median / p99 / pooled ratio: {q[0]:.2f} ({q[1]}); bound K_QUANTILE = {M.K[0]:g}")
    print(f"largest maximum ratio: {mx[0]:.2f} ({mx[1]}); bound K_MAX = {M.K[1]:g}")
    print("\n## The judged cells (float64 reference alone)\n")
    print("| case | level | e32 = max abs(v32 - v64) | cells | left out by the ambiguity band | judged | most tiles listing / contributing to a point |")
    print("|---|---|---|---|---|---|---|")
    import numpy as np
    for c in M.CASES:
        _, _, _, b64, b32, live, level = M.reference(c)
        amb, judged = M.judged(c)
        e32 = float(np.abs(b32["v"].astype(np.float64) - b64["v"])[live].max())
        print(f"| {M.case_id(c)} | {level:.6g} | {e32:.3g} | {judged.size} | {judged.size - int(judged.sum())} | {int(judged.sum())} | "
              f"{int(b64['listed'].max())} / {int(b64['run'].max())} |")


if __name__ == "__main__":
    main(sys.argv[1])
