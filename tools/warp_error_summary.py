"""The table of profiles/warp_error.md from the log of `pytest tests/test_gpu_warp_edges.py -m gpu -s`: one row per judged
quantity (kernel's and float32 yardstick's median / p99 / max / pooled, and the ratios against the yardstick floored at 2^-24, as
warp_cases.judge bounds them), then the largest ratios and the margins they give (doubled, rounded up to a power of two)."""
import math
import re
import sys

FLOOR = 2.0 ** -24
LINE = re.compile(r"^[.F]*(.+?): op (.+?) \| f32 ref (.+?) \| ratio ")


def main(path):
    rows = []
    for line in open(path):
        m = LINE.match(line.strip())
        if not m:
            continue
        op = [float(x) for x in m.group(2).split(" / ")]
        ref = [float(x) for x in m.group(3).split(" / ")]
        rows.append((m.group(1), op, ref, [0.0 if a == 0 else a / max(b, FLOOR) for a, b in zip(op, ref)]))
    print("| case and quantity | kernel: median / p99 / max / pooled | float32 yardstick | ratio (yardstick floored at 2^-24) |")
    print("|---|---|---|---|")
    fmt = lambda v, f: " / ".join(f % x for x in v)
    for name, op, ref, ratio in rows:
        print(f"| {name} | {fmt(op, '%.2e')} | {fmt(ref, '%.2e')} | {fmt(ratio, '%.2f')} |")
    quant = max(rows, key=lambda r: max(r[3][0], r[3][1], r[3][3]))
    worst = max(rows, key=lambda r: r[3][2])
    k = lambda x: 2.0 ** math.ceil(math.log2(2 * x))
    q = max(quant[3][0], quant[3][1], quant[3][3])
    print(f"\n- {len(rows)} judged quantities")
    print(f"- largest median / p99 / pooled ratio: {q:.2f} ({quant[0]}) -> K_QUANTILE = {k(q):.0f}")
    print(f"- largest maximum ratio: {worst[3][2]:.2f} ({worst[0]}) -> K_MAX = {k(worst[3][2]):.0f}")


if __name__ == "__main__":
    main(sys.argv[1])
