#!/usr/bin/env python3
"""The judge() lines of `pytest -m gpu -s tests/test_gpu_mesh_extract.py > mesh.log` as the markdown table of
profiles/mesh_extract_error.md, with the largest ratios and the margins they give (doubled, rounded up to a power of two).  A ratio
is the kernel's figure over max(float32 yardstick's figure, 2^-24), which is how tests/surface_nets_reference.py forms every bound;
the quantile figures of cases with fewer than 16 vertices do not bind and are left out of that maximum (their lines carry the same
four figures; the test binds only the maximum and the pooled one).

    python tools/mesh_extract_error_summary.py mesh.log > table.md"""
import math
import re
import sys

FLOOR = 2.0 ** -24
LINE = re.compile(r"^[.F]*(.+?): op (.+?) \| f32 ref (.+?) \| ratio")


def main(path):
    rows, seen = [], set()
    for ln in open(path):
        m = LINE.match(ln.strip())
        if m and m.group(1) not in seen:
            seen.add(m.group(1))
            a, b = ([float(v) for v in m.group(k).split(" / ")] for k in (2, 3))
            rows.append((m.group(1), m.group(2), m.group(3), [x / max(y, FLOOR) for x, y in zip(a, b)]))
    print("| case and tensor | kernel: median / p99 / max / pooled | float32 yardstick | ratios (yardstick floored at 2^-24) |")
    print("|---|---|---|---|")
    for name, op, ref, r in rows:
        print(f"| {name} | {op} | {ref} | " + " / ".join(f"{v:.2f}" for v in r) + " |")
    q = max((max(r[0], r[1], r[3]), n) for n, _, _, r in rows)
    mx = max((r[2], n) for n, _, _, r in rows)
    up = lambda v: 2.0 ** math.ceil(math.log2(2.0 * v)) if v > 0 else 1.0
    print(f"\nlargest median / p99 / pooled ratio: {q[0]:.2f} ({q[1]}) -> K_QUANTILE = {up(q[0]):g}")
    print(f"largest maximum ratio: {mx[0]:.2f} ({mx[1]}) -> K_MAX = {up(mx[0]):g}")


if __name__ == "__main__":
    main(sys.argv[1])
