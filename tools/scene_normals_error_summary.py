#!/usr/bin/env python3
"""The judge() lines of `pytest -m gpu -s tests/test_gpu_scene_normals.py > normals.log` as the markdown table of
profiles/scene_normals_error.md: per judged case and tensor the float32 yardstick's figures, the kernel's, their ratios (the yardstick's
figure taken as at least 2^-24, as tests/scene_normals_reference.py forms every bound) and the share of contributing points whose unit
normal is judged.  K is normals_reference's figure: it is read here, never derived from this run.

    python tools/scene_normals_error_summary.py normals.log > profiles/scene_normals_error.md"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

FLOOR = 2.0 ** -24
LINE = re.compile(r"^[.F]*(.+?): op (.+?) \| f32 ref (.+?) \| ratio")
SHARE = re.compile(r"^[.F]*(.+?) normal: (\d+) of (\d+) contributing points judged \(share left out ([0-9.]+)\)")


def main(path):
    import scene_normals_reference as R
    rows, seen, share = [], set(), {}
    for ln in open(path):
        s = SHARE.match(ln.strip())
        if s:
            share[s.group(1)] = (int(s.group(2)), int(s.group(3)), float(s.group(4)))
        m = LINE.match(ln.strip())
        if m and m.group(1) not in seen:
            seen.add(m.group(1))
            a, b = ([float(v) for v in m.group(k).split(" / ")] for k in (2, 3))
            rows.append((m.group(1), m.group(2), m.group(3), [x / max(y, FLOOR) for x, y in zip(a, b)]))
    print("# Blended density gradient: the fused op against float64 (tests/test_gpu_scene_normals.py on an MI355X)\n")
    print("sigma equals the scene mesh's field at the lattice points, and sigma and grad equal the composed route, bit for bit in every "
          "case (the tests assert it).  grad is |g - g64|_2 over the conditioning scale |cond|_2 at EVERY point of the list (points no tile "
          "contributes to: error 0); normal is |n - n64|_2 at the judged points.\n")
    print("| case and tensor | float32 yardstick: median / p99 / max / pooled | kernel | ratios (yardstick floored at 2^-24) | normals judged / contributing points (share left out) |")
    print("|---|---|---|---|---|")
    for name, op, ref, r in rows:
        case = name.rsplit(" ", 1)[0]
        sh = share.get(case)
        col = f"{sh[0]} / {sh[1]} ({sh[2]:.4f})" if sh and name.endswith("normal") else ""
        print(f"| {name} | {ref} | {op} | " + " / ".join(f"{v:.2f}" for v in r) + f" | {col} |")
    q = max((max(r[0], r[1], r[3]), n) for n, _, _, r in rows)
    mx = max((r[2], n) for n, _, _, r in rows)
    print(f"\nlargest median / p99 / pooled ratio: {q[0]:.2f} ({q[1]}); bound K_QUANTILE = {R.K[0]:g}")
    print(f"largest maximum ratio: {mx[0]:.2f} ({mx[1]}); bound K_MAX = {R.K[1]:g}")
    print(f"\nThe share of contributing points without a judged normal is capped at {R.N_CAP:g} on the reference alone; the EDGES (a "
          "handful of points, one of them with W == 0 and g == 0 on purpose) are capped pooled with their scene's random points "
          "(tests/test_scene_normals_cpu.py).")


if __name__ == "__main__":
    main(sys.argv[1])
