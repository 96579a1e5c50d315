#!/usr/bin/env python3
"""Device-resident time of vgt_hip_fill_enclosed_dev on grids of hollow spheres (synthetic.hollow_spheres), interleaved in
one process with vgt_hip_connected_components_dev on the same grid -- the labelling the fill shares its first two
kernels with, and the yardstick of DESIGN.md 4d: the fill's median must not lie above the labelling's.

  python tools/bench_fill.py [--sizes 256 512 1024] [--steps 20] [--warmup 3] [--out profiles/fill/bench_fill.json]
  python tools/bench_fill.py --sizes 1024 --only-fill --steps 3 --warmup 1     what a kernel trace should see

Timing: wall clock around the call (both calls end with the read-back of a count, so the stream is drained; a
vgt_hip_synchronize before brackets it), `steps` repetitions after `warmup`, median and min / max.  Every step of the fill
runs on a fresh device copy of the input; the copy is finished before the clock starts.  One JSON line per size.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(ms):
    ms = np.asarray(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4),
            "max_ms": round(float(ms.max()), 4), "steps": int(ms.size)}


def main():
    import torch
    from voxelized_geometry_tools_amd import capi, synthetic

    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only-fill", action="store_true", help="skip the labelling (for a kernel trace of the fill alone)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    ctx = capi.Context(0)
    for size in args.sizes:
        shape = (size, size, size)
        occ_dev = torch.from_numpy(synthetic.hollow_spheres(shape, seed=42)).cuda()
        work_dev = torch.empty_like(occ_dev)
        labels_dev = None if args.only_fill else torch.empty(shape, dtype=torch.int32, device="cuda")
        fill_ms, label_ms, filled, components = [], [], 0, 0
        for step in range(args.warmup + args.steps):
            work_dev.copy_(occ_dev)
            torch.cuda.synchronize()
            ctx.synchronize()
            t0 = time.perf_counter()
            filled = ctx.fill_enclosed_dev(work_dev.data_ptr(), 4, shape)
            t1 = time.perf_counter()
            if step >= args.warmup:
                fill_ms.append((t1 - t0) * 1e3)
            if args.only_fill:
                continue
            ctx.synchronize()
            t0 = time.perf_counter()
            components = ctx.connected_components_dev(occ_dev.data_ptr(), shape, labels_dev.data_ptr())
            t1 = time.perf_counter()
            if step >= args.warmup:
                label_ms.append((t1 - t0) * 1e3)
        rec = {"case": "fill_enclosed_dev", "dist": "hollow_spheres", "shape": list(shape), "filled": filled,
               "shell_cells": int((occ_dev > 0.5).sum().item())}
        rec.update(_stats(fill_ms))
        rec["voxels_per_s"] = round(size ** 3 / (rec["median_ms"] * 1e-3), 1)
        if not args.only_fill:
            rec["components"] = components
            rec["labelling"] = _stats(label_ms)
            rec["ratio_to_labelling"] = round(rec["median_ms"] / rec["labelling"]["median_ms"], 3)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del occ_dev, work_dev, labels_dev
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
