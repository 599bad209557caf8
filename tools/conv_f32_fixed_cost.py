"""Fixed cost per workgroup of the 128-filter direct f32 tile, from per-layer tables of tools/yolo_layer_table.py (developer tool).
usage: conv_f32_fixed_cost.py <layers.txt> [<layers.txt> ...]

A layer of s K steps (s = taps * cin / 16) runs at rate = A * s / (s + c): c is what a workgroup spends outside its K loop (set-up, prologue,
epilogue), in units of one K step.  A = 145 TFLOP/s is the long-K asymptote of the <16, 2, 2, 4> tile.  Prints, per shape class (layers of
one kernel size, stride, channel counts and map size), the mean time and rate of its layers and the implied c, one column pair per table."""
import re
import sys
from collections import OrderedDict

A = 145.0
ROW = re.compile(r"^L\s*(\d+) (\d)x\d/(\d)\s+(\d+)->\s*(\d+)\s+(\d+)x\s*(\d+)\s+(.{22}) grid.*?([\d.]+) us\s+([\d.]+) TFLOP/s")


def classes(path):
    out = OrderedDict()
    for line in open(path):
        m = ROW.match(line)
        if not m or "k_conv_f32<16, 2" not in m.group(8):
            continue
        k, st, cin, f, wo, ho = (int(m.group(i)) for i in (2, 3, 4, 5, 6, 7))
        out.setdefault((k, st, cin, f, wo, ho), []).append((float(m.group(9)), float(m.group(10))))
    return out


def main():
    tabs = [classes(p) for p in sys.argv[1:]]
    print("A = %.0f TFLOP/s; columns per table: %s" % (A, ", ".join(sys.argv[1:])))
    print("%-28s %6s %3s  %s" % ("shape class", "s", "n", "   ".join("us/layer  TFLOP/s      c" for _ in tabs)))
    for key in tabs[0]:
        k, st, cin, f, wo, ho = key
        s = k * k * cin // 16
        cols = []
        for t in tabs:
            rows = t.get(key, [])
            us = sum(r[0] for r in rows) / max(len(rows), 1)
            rate = sum(r[1] for r in rows) / max(len(rows), 1)
            cols.append("%8.1f %8.1f %6.1f" % (us, rate, s * (A / rate - 1.0) if rate else float("nan")))
        print("%dx%d/%d %4d->%4d %3dx%-3d %8d %3d  %s" % (k, k, st, cin, f, wo, ho, s, len(tabs[0][key]), "   ".join(cols)))
    for p, t in zip(sys.argv[1:], tabs):
        print("%s: %.2f ms in the %d layers of this tile" % (p, sum(r[0] for rows in t.values() for r in rows) / 1e3, sum(len(r) for r in t.values())))


if __name__ == "__main__":
    main()
