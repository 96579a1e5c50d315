#!/usr/bin/env python3
"""Condenses the raw lines of tools/ab_libs.sh (or tools/ab_shape.py) runs: per library min - max (median) of ms_per_step and
of the X kernel, and the two tests a gain has to pass against the first library (every run below every run of it; median
difference at least twice its spread).  Usage: python tools/ab_summary.py FILE ..."""
import ast
import re
import statistics
import sys


def parse(path):
    runs = {}
    for line in open(path):
        fields = line.split()
        if not fields or not fields[0].startswith("libvgt"):
            continue
        lib = fields[0]
        if "{" in line:  # ab_libs.sh: lib, bench args, ms_per_step, kernel dict
            kernels = ast.literal_eval(line[line.index("{"):])
            step = float(line[:line.index("{")].split()[-1])
            x = kernels["PassXFinalize"]
        else:            # ab_shape.py: ... X <ms> sum <ms>
            x = float(re.search(r"X ([0-9.]+)", line).group(1))
            step = float(re.search(r"sum ([0-9.]+)", line).group(1))
        runs.setdefault(lib, {"step": [], "x": []})
        runs[lib]["step"].append(step)
        runs[lib]["x"].append(x)
    return runs


def main():
    for path in sys.argv[1:]:
        runs = parse(path)
        libs = list(runs)
        print("## %s" % path)
        for key, label in (("x", "X kernel"), ("step", "ms_per_step (ab_shape: kernel sum)")):
            base = runs[libs[0]][key]
            spread = max(base) - min(base)
            for lib in libs:
                v = runs[lib][key]
                print("%-22s %-34s %.4f - %.4f (median %.4f), %d runs" % (lib, label, min(v), max(v), statistics.median(v), len(v)))
            for lib in libs[1:]:
                v = runs[lib][key]
                diff = statistics.median(base) - statistics.median(v)
                print("  %s against %s, %s: every run below every run: %s; median difference %+.4f ms (%+.2f %%) against twice "
                      "the first library's spread %.4f: %s; median not above the first's median + spread: %s" % (
                          lib, libs[0], label, max(v) < min(base), -diff, -100 * diff / statistics.median(base), 2 * spread,
                          diff >= 2 * spread, statistics.median(v) <= statistics.median(base) + spread))


if __name__ == "__main__":
    main()
