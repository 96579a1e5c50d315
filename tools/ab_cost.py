#!/usr/bin/env python3
"""A/B of builds of the clearance-cost kernel (csrc/cost_kernels.hip) that differ in a compile-time knob --
VGT_COST_BUFFER_PASSES, VGT_COST_TILE_BYTES, VGT_COST_MAX_TILE --: tools/bench_cost.py --call-only once per library and
round, each in a process of its own (VGT_HIP_LIB names the library), the libraries alternating within a round so that a
drift of the machine shows as a difference between the rounds and not between the builds.

  python tools/ab_cost.py --libs P1=/path/libvgt_hip_P1.so P4=voxelized_geometry_tools_amd/libvgt_hip.so ... \\
                          --out profiles/cost/ab/buffer_passes.json [--rounds 2] [--batches 100000] [--spheres 16 64 200]

A variant library: cost_kernels.hip compiled with the build's flags plus e.g. -DVGT_COST_BUFFER_PASSES=8 and linked
with the other objects of csrc/Makefile.  Every run first compares the call with the composed route bit for bit.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--libs", nargs="+", required=True, help="NAME=PATH ...")
    parser.add_argument("--out", required=True)
    parser.add_argument("--rounds", type=int, default=2)
    parser.add_argument("--size", type=int, default=512)
    parser.add_argument("--batches", nargs="+", default=["100000"])
    parser.add_argument("--spheres", nargs="+", default=["16", "64", "200"])
    parser.add_argument("--trees", nargs="+", default=["arm", "body"])
    parser.add_argument("--timeout", type=int, default=240)
    args = parser.parse_args()
    rows = []
    for round_index in range(args.rounds):
        for item in args.libs:
            name, path = item.split("=", 1)
            with tempfile.TemporaryDirectory() as scratch:
                out = os.path.join(scratch, "rows.json")
                command = [sys.executable, os.path.join(ROOT, "tools", "bench_cost.py"), "--call-only", "--size",
                           str(args.size), "--out", out, "--batches"] + args.batches + ["--spheres"] + args.spheres + \
                          ["--trees"] + args.trees
                done = subprocess.run(command, env=dict(os.environ, VGT_HIP_LIB=os.path.abspath(path)),
                                      stdout=subprocess.DEVNULL, timeout=args.timeout)
                if done.returncode != 0:
                    sys.exit("%s: bench_cost.py ended with %d; nothing more is started" % (name, done.returncode))
                for row in json.load(open(out)):
                    row.update(build=name, round=round_index)
                    rows.append(row)
                    print(json.dumps({k: row[k] for k in ("build", "round", "tree", "configurations", "spheres", "margin")}
                                     | {"cost_ms": row["cost_ms"]["median_ms"],
                                        "cost_only_ms": row["cost_only_ms"]["median_ms"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
