#!/usr/bin/env python3
"""Condense the figures tests/test_gpu_toy_limits.py prints into profiles/toy_limits_parity.txt:

    python -m pytest -m gpu -s tests/test_gpu_toy_limits.py | python tools/toy_limits_report.py > profiles/toy_limits_parity.txt

One row per (case, batch, first-layer form or route); a cell is `max/rms|max/rms` -- the kernel's error against float64,
then the float32 oracle's own -- or a single relative max error where the test has no float32 yardstick."""
import collections
import re
import sys

ROW = re.compile(r"toy_limits (\S+)\s+B=(\d+)\s+(\S+)\s+(\S+)\s+(?:max (\S+) rms (\S+) \| fp32 oracle max (\S+) rms (\S+)"
                 r"|rel max (\S+)|max (\S+) \| layered-f64 (\S+) one-f64 (\S+))")
TARGET = re.compile(r"toy_limits target (\S+) rows=(\d+)\s+T=(\S+) (\S+)\s+rel max (\S+)")


def main():
    rows, targets = collections.OrderedDict(), collections.OrderedDict()
    for line in sys.stdin:
        m = TARGET.search(line)
        if m:
            targets.setdefault(m.group(1, 2, 3), []).append(f"{m.group(4)} {m.group(5)}")
            continue
        m = ROW.search(line)
        if not m:
            continue
        case, B, what, name = m.group(1, 2, 3, 4)
        if m.group(5):
            cell = f"{name} {m.group(5)}/{m.group(6)}|{m.group(7)}/{m.group(8)}"
        elif m.group(9):
            cell = f"{name} {m.group(9)}"
        else:
            cell = f"{name} {m.group(10)} (layered-f64 {m.group(11)}, one-launch-f64 {m.group(12)})"
        rows.setdefault((case, B, what), []).append(cell)
    print("Toy-target one-launch kernels at their stated limits against float64 (tests/test_gpu_toy_limits.py, MI355X).")
    print("cell: output max/rms|float32-oracle max/rms (sampling outputs: relative to max(1, |reference|max), p absolute);")
    print("      a single figure is a max error relative to the reference tensor's largest entry (gradients, target entries).")
    print("case: d<x_dim>-K<components><g Gaussian | m mixture>-H<num_nodes>-N<leapfrog steps>-<weight regime>[-T<temperature>]")
    print()
    for (case, B, what), cells in rows.items():
        print(f"{case:<26s} B={B:<3s} {what:<12s} " + "  ".join(cells))
    print()
    for (case, n, T), cells in targets.items():
        print(f"target {case:<8s} rows={n:<4s} T={T:<4s} " + "  ".join(cells))


if __name__ == "__main__":
    main()
