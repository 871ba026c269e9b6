#!/usr/bin/env python3
"""The judge() lines of `pytest -m gpu -s tests/test_gpu_render_normals.py > render_normals.log` as the markdown table of
profiles/render_normals_error.md, with the largest ratios.  A ratio is the kernel's figure over max(float32 yardstick's figure,
2^-24), which is how tests/render_normals_reference.py forms every bound (K = 8 on each of median, 99th percentile, maximum and
pooled; no sample and no ray left out).

    python tools/render_normals_error_summary.py render_normals.log > table.md"""
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
    print("| case | kernel: median / p99 / max / pooled | float32 yardstick | ratios (yardstick floored at 2^-24) |")
    print("|---|---|---|---|")
    for name, op, ref, r in rows:
        print(f"| {name} | {op} | {ref} | " + " / ".join(f"{v:.2f}" for v in r) + " |")
    q = max((max(r[0], r[1], r[3]), n) for n, _, _, r in rows)
    mx = max((r[2], n) for n, _, _, r in rows)
    print(f"\nlargest median / p99 / pooled ratio: {q[0]:.2f} ({q[1]}); largest maximum ratio: {mx[0]:.2f} ({mx[1]}); bound: K = 8 on each")


if __name__ == "__main__":
    main(sys.argv[1])
