#!/usr/bin/env python3
"""The judge() lines of `pytest -m gpu -s tests/test_gpu_render_infer_error.py > render_infer.log` as the tables of
profiles/render_infer_error.md: one row per op, route, case and quantity (the op's median / p99 / max / pooled error against float64,
the float32 yardstick's own, the ratios), then per op and route the largest ratios -- which is what the K of
tests/render_infer_reference.py are held against (K_SPLIT = 8 is given; K_F32 and K_ACC are the largest ratio, doubled and rounded
up to a power of two) -- and per family and route the median and maximum error of DESIGN.md's table.  A ratio is the op's figure over
max(float32 yardstick's figure, 2^-24), which is how every bound is formed.

    python tools/render_infer_error_summary.py render_infer.log > tables.md"""
import collections
import re
import sys

FLOOR = 2.0 ** -24
LINE = re.compile(r"^[.F]*(.+?): op (.+?) \| f32 ref (.+?) \| ratio")
FAMILIES = ("base", "dense", "thin", "bias", "wide", "fresh", "zero", "axis", "face", "long", "short")


def route_of(name):
    """(op, route) of a judge line's name: "pts_inference G9-17-base plain layout 1 dif abs" -> ("pts_inference", "plain")"""
    w = name.split()
    known = [r for r in ("default", "plain", "h3", "f32", "skip") if r in w[2:]]
    if w[0] == "pts_inference" and "G65" in w[1] or w[0] == "bg_pts_inference_v2" and "G65" in w[1]:
        return w[0], "f32 (above 64 tiles)"
    return w[0], {"skip": "fused slot lists"}.get(known[0], known[0]) if known else "-"


def main(path):
    rows, seen = [], set()
    for ln in open(path):
        m = LINE.match(ln.strip())
        if m and m.group(1) not in seen:
            seen.add(m.group(1))
            a, b = ([float(v) for v in m.group(k).split(" / ")] for k in (2, 3))
            rows.append((m.group(1), a, b, [x / max(y, FLOOR) for x, y in zip(a, b)]))
    fmt = lambda v: " / ".join(f"{x:.2e}" for x in v)
    print("| op, case, route, quantity | op: median / p99 / max / pooled | float32 yardstick | ratios (yardstick floored at 2^-24) |")
    print("|---|---|---|---|")
    for name, a, b, r in rows:
        print(f"| {name} | {fmt(a)} | {fmt(b)} | " + " / ".join(f"{v:.2f}" for v in r) + " |")

    worst = collections.OrderedDict()
    for name, a, b, r in rows:
        key = route_of(name)
        q, mx = max(r[0], r[1], r[3]), r[2]
        cur = worst.setdefault(key, [(0.0, ""), (0.0, "")])
        if q > cur[0][0]:
            cur[0] = (q, name)
        if mx > cur[1][0]:
            cur[1] = (mx, name)
    print("\n| op | route | largest median / p99 / pooled ratio | at | largest maximum ratio | at |")
    print("|---|---|---|---|---|---|")
    for (op, route), (q, mx) in worst.items():
        print(f"| {op} | {route} | {q[0]:.2f} | {q[1]} | {mx[0]:.2f} | {mx[1]} |")

    fam = collections.OrderedDict()
    for name, a, b, r in rows:
        w = name.split()
        if w[0] not in ("pts_inference", "bg_pts_inference_v2") or not name.endswith("abs"):
            continue
        f = w[1].split("-")[-1]
        if f in FAMILIES:
            cur = fam.setdefault((f, route_of(name)[1]), [0.0, 0.0, 0.0, 0.0])
            cur[0], cur[1], cur[2], cur[3] = max(cur[0], a[0]), max(cur[1], a[2]), max(cur[2], b[0]), max(cur[3], b[2])
    print("\n| family | route | op: largest median | largest maximum | float32 yardstick: largest median | largest maximum |")
    print("|---|---|---|---|---|---|")
    for (f, route), v in sorted(fam.items(), key=lambda kv: (FAMILIES.index(kv[0][0]), kv[0][1])):
        print(f"| {f} | {route} | {v[0]:.2e} | {v[1]:.2e} | {v[2]:.2e} | {v[3]:.2e} |")


if __name__ == "__main__":
    main(sys.argv[1])
