#!/usr/bin/env python3
"""Device-resident time of the nearest-other-class transform (vgt_hip_nearest_dev) beside vgt_hip_sdf_dev on the same
grid, in the same process, the two alternating.  One JSON line per case.

  python tools/bench_nearest.py [--sizes 256 512 1024] [--dists spheres salt] [--reps 10] [--rounds 5] [--warmup 2]
                                [--out profiles/nearest/bench_nearest.json]

Timing: device events on the context's stream around `reps` back-to-back calls, `rounds` such windows per variant after
`warmup` calls of each; the variants (nearest, nearest with d2, the SDF) take turns round by round.  Reported per call:
median, min and max over the rounds.
Floor convention: the three passes must move 20 B/voxel (4 read, 2 + 2 for the Z pass, 4 + 4 for the Y pass, 4
written; 4 more with d2) at the HBM peak of 8000 GB/s.  The stack traffic of the line passes and their second read of
every line are what the design adds on top.
Every case also checks, on the device, that sqrt(d2) * resolution (negated in filled cells) is the SDF's field bit for bit.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0
RESOLUTION = 0.02


def _stats(ms, prefix):
    ms = np.asarray(ms)
    return {prefix + "median_ms": round(float(np.median(ms)), 4), prefix + "min_ms": round(float(ms.min()), 4),
            prefix + "max_ms": round(float(ms.max()), 4)}


def main():
    import torch
    from voxelized_geometry_tools_amd import capi, synthetic

    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--dists", nargs="+", default=["spheres", "salt"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(record):
        line = json.dumps(record)
        print(line, flush=True)
        lines.append(line)
        if args.out:  # (rewritten after every case: a run that is cut short keeps what it measured)
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    for size in args.sizes:
        shape = (size, size, size)
        vox = size ** 3
        ws_bytes = capi.nearest_workspace_bytes(shape)
        sdf_ws_bytes = capi.sdf_workspace_bytes(shape)
        nearest = torch.empty(vox, dtype=torch.int32, device="cuda")
        d2 = torch.empty(vox, dtype=torch.int32, device="cuda")
        sdf = torch.empty(vox, dtype=torch.float32, device="cuda")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        sdf_ws = torch.empty(sdf_ws_bytes, dtype=torch.uint8, device="cuda")
        for dist in args.dists:
            occ = torch.from_numpy(synthetic.make_occupancy(shape, dist, seed=42)).cuda()
            torch.cuda.synchronize()
            variants = {
                "nearest": lambda: ctx.nearest_dev(occ.data_ptr(), shape, nearest.data_ptr(), ws.data_ptr(), ws_bytes),
                "nearest_d2": lambda: ctx.nearest_dev(occ.data_ptr(), shape, nearest.data_ptr(), ws.data_ptr(), ws_bytes,
                                                      d2_ptr=d2.data_ptr()),
                "sdf": lambda: ctx.sdf_dev(occ.data_ptr(), shape, RESOLUTION, sdf.data_ptr(), sdf_ws.data_ptr(),
                                           sdf_ws_bytes),
            }
            for call in variants.values():
                for _ in range(args.warmup):
                    call()
            ctx.synchronize()
            ms = {name: [] for name in variants}
            for _ in range(args.rounds):
                for name, call in variants.items():
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record(stream)
                    for _ in range(args.reps):
                        call()
                    stop.record(stream)
                    stop.synchronize()
                    ms[name].append(start.elapsed_time(stop) / args.reps)
            # d2 against the SDF of the same grid, on the device
            filled = occ.reshape(-1) >= 0.5
            want = (torch.sqrt(d2.double()) * RESOLUTION).float()
            want = torch.where(filled, -want, want)
            equal = bool(torch.equal(want.view(torch.int32), sdf.view(torch.int32)))
            in_range = bool(((nearest >= 0) & (nearest < vox)).all())
            other_class = bool((filled[nearest.long().clamp(0, vox - 1)] != filled).all())
            rec = {"case": "nearest_dev", "dist": dist, "shape": list(shape), "filled_fraction": round(float(filled.float().mean()), 6),
                   "reps_per_window": args.reps, "windows": args.rounds, "workspace_bytes": ws_bytes,
                   "sdf_workspace_bytes": sdf_ws_bytes}
            for name in variants:
                rec.update(_stats(ms[name], name + "_"))
            rec["nearest_over_sdf"] = round(rec["nearest_median_ms"] / rec["sdf_median_ms"], 3)
            rec["nearest_d2_over_sdf"] = round(rec["nearest_d2_median_ms"] / rec["sdf_median_ms"], 3)
            rec["floor"] = "20 B/voxel (24 with d2) at %g GB/s" % HBM_PEAK_GBPS
            rec["nearest_fraction_of_hbm_floor"] = round(20 * vox / (rec["nearest_median_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)
            rec["nearest_d2_fraction_of_hbm_floor"] = round(24 * vox / (rec["nearest_d2_median_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)
            rec["voxels_per_s"] = round(vox / (rec["nearest_median_ms"] * 1e-3), 1)
            rec["d2_reproduces_sdf_bitwise"] = equal
            rec["targets_in_grid_and_of_other_class"] = in_range and other_class
            emit(rec)
            del occ, filled, want
        del nearest, d2, sdf, ws, sdf_ws
        torch.cuda.empty_cache()
    ctx.reset_stream()
    ctx.close()


if __name__ == "__main__":
    main()
