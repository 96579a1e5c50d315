#!/usr/bin/env python3
"""A/B of builds of the motion check with the self part (csrc/motion_self_kernels.hip) that differ in a compile-time knob
-- VGT_MOTION_SELF_TILE_BYTES --, by the protocol of tools/ab_self.py: tools/bench_motion_self.py --call-only once per
library and round, each in a process of its own (VGT_HIP_LIB names the library), the libraries alternating within a round
so that a drift of the machine shows as a difference between the rounds and not between the builds.

  python tools/ab_motion_self.py --libs T8=/path/libvgt_hip_T8.so T16=voxelized_geometry_tools_amd/libvgt_hip.so ... \\
                                 --out profiles/motion_self/ab/tile_bytes.json [--rounds 2] [--shapes 10000x99 100000x9]

A variant library: motion_self_kernels.hip compiled with the build's flags plus e.g. -DVGT_MOTION_SELF_TILE_BYTES=8192
and linked with the other objects of csrc/Makefile.  Every run first compares the call with the composed route.
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
    parser.add_argument("--shapes", nargs="+", default=["10000x99", "100000x9"])
    parser.add_argument("--spheres", nargs="+", default=["16", "64", "200"])
    parser.add_argument("--trees", nargs="+", default=["arm", "body"])
    parser.add_argument("--size", default="512")
    parser.add_argument("--timeout", type=int, default=240)
    args = parser.parse_args()
    rows = []
    for round_index in range(args.rounds):
        for item in args.libs:
            name, path = item.split("=", 1)
            with tempfile.TemporaryDirectory() as scratch:
                out = os.path.join(scratch, "rows.json")
                command = [sys.executable, os.path.join(ROOT, "tools", "bench_motion_self.py"), "--call-only",
                           "--out", out, "--size", args.size, "--shapes"] + args.shapes + ["--spheres"] + args.spheres + \
                          ["--trees"] + args.trees
                done = subprocess.run(command, env=dict(os.environ, VGT_HIP_LIB=os.path.abspath(path)),
                                      stdout=subprocess.DEVNULL, timeout=args.timeout)
                if done.returncode != 0:
                    sys.exit("%s: bench_motion_self.py ended with %d; nothing more is started" % (name, done.returncode))
                for row in json.load(open(out)):
                    row.update(build=name, round=round_index)
                    rows.append(row)
                    shown = ("build", "round", "tree", "motions", "steps_per_motion", "spheres", "stop_at_collision",
                             "tile_samples")
                    print(json.dumps({k: row[k] for k in shown} | {"call_ms": row["call_ms"]["median_ms"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(row) for row in rows) + "\n]\n")   # (one row per line)


if __name__ == "__main__":
    main()
