#!/usr/bin/env python3
"""The judge() lines of `pytest -m gpu -s tests/test_gpu_per_ray_ops.py > per_ray.log` as the markdown table of
profiles/per_ray_ops_error.md, with the largest ratios and the margins they give (doubled, rounded up to a power of two).

    python tools/per_ray_error_summary.py per_ray.log > table.md"""
import math
import re
import sys

LINE = re.compile(r"^[.F]*(.+?): op (.+?) \| f32 ref (.+?) \| ratio ([0-9.einf /]+?)(  \[few rays.*)?$")


def main(path):
    rows, seen = [], set()
    for ln in open(path):
        m = LINE.match(ln.strip())
        if m and m.group(1) not in seen:
            seen.add(m.group(1))
            rows.append((m.group(1), m.group(2), m.group(3), [float(v) for v in m.group(4).split(" / ")], bool(m.group(5))))
    print("| case and tensor | op: median / p99 / max / pooled | float32 reference | ratios |")
    print("|---|---|---|---|")
    for name, op, ref, r, few in rows:
        print(f"| {name}{' (few rays)' if few else ''} | {op} | {ref} | " + " / ".join(f"{v:.2f}" for v in r) + " |")
    finite = [(n, r) for n, _, _, r, few in rows if not few and not n.startswith("thin-") and all(math.isfinite(v) for v in r)]   # (a handful of rays: a ratio of two roundings; thin rays: the stated __expf finding)
    q = max(finite, key=lambda t: max(t[1][0], t[1][1], t[1][3]))
    mx = max(finite, key=lambda t: t[1][2])
    up = lambda v: 2.0 ** math.ceil(math.log2(2.0 * v))
    qv, mv = max(q[1][0], q[1][1], q[1][3]), mx[1][2]
    print(f"\nlargest median / p99 / pooled ratio: {qv:.2f} ({q[0]}) -> K_QUANTILE = {up(qv):g}")
    print(f"largest maximum ratio: {mv:.2f} ({mx[0]}) -> K_MAX = {up(mv):g}")


if __name__ == "__main__":
    main(sys.argv[1])
