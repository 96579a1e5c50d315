#!/usr/bin/env python3
"""Device-resident time of the component labelling (vgt_hip_connected_components_dev) and of the spatial-segment chain,
beside the CPU yardsticks of tests/components_ref.py.  One JSON line per case.

  python tools/bench_components.py [--sizes 256 512 1024] [--steps 20] [--warmup 3] [--no-cpu] [--out FILE]
  python tools/bench_components.py --topology [--sizes 256 1024] [--dists spheres] ...   the component topology
      (vgt_hip_component_topology_dev) on labelled grids, beside the labelling of the same grid

Timing: wall clock around the call (it ends with the read-back of the count, so the stream is drained; a
vgt_hip_synchronize before and after brackets it), `steps` repetitions after `warmup`, median and min / max.
Floor convention: the plain entry point must read 4 B/voxel of occupancy and write 4 B/voxel of labels = 8 B/voxel at the
HBM peak of 8000 GB/s; everything the union-find and the scan move in between is scratch traffic the design is judged by.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBPS = 8000.0
FLOOR_BYTES_PER_VOXEL = 8


def _stats(ms):
    ms = np.asarray(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4),
            "max_ms": round(float(ms.max()), 4), "steps": int(ms.size)}


def _timed(ctx, call, warmup, steps):
    ms, result = [], None
    for step in range(warmup + steps):
        ctx.synchronize()
        t0 = time.perf_counter()
        result = call()
        ctx.synchronize()
        if step >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms, result


def bench_topology(ctx, args, emit):
    """vgt_hip_component_topology_dev (all classes) on device-resident labels; the labelling of the same grid as the
    yardstick.  Both calls block (each reads a count / the table back)."""
    import torch
    from voxelized_geometry_tools_amd import synthetic
    for size in args.sizes:
        shape = (size, size, size)
        for dist in args.dists:
            occ_dev = torch.from_numpy(synthetic.make_occupancy(shape, dist, seed=42)).cuda()
            labels_dev = torch.empty(shape, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            label_ms, count = _timed(ctx, lambda: ctx.connected_components_dev(occ_dev.data_ptr(), shape,
                                                                               labels_dev.data_ptr()),
                                     args.warmup, args.steps)
            topo_ms, table = _timed(ctx, lambda: ctx.component_topology_dev(occ_dev.data_ptr(), labels_dev.data_ptr(),
                                                                            shape, 7, count),
                                    args.warmup, args.steps)
            rec = {"case": "component_topology_dev", "dist": dist, "shape": list(shape), "components": count,
                   "component_types": 7, "surface_nodes": int(table["num_surface_vertices"].sum()),
                   "max_holes": int(table["num_holes"].max()), "max_voids": int(table["num_voids"].max())}
            rec.update(_stats(topo_ms))
            rec["labelling_median_ms"] = _stats(label_ms)["median_ms"]
            rec["ratio_to_labelling"] = round(rec["median_ms"] / rec["labelling_median_ms"], 3)
            rec["voxels_per_s"] = round(size ** 3 / (rec["median_ms"] * 1e-3), 1)
            emit(rec)
            del occ_dev, labels_dev


def main():
    import torch
    import components_ref as R
    from voxelized_geometry_tools_amd import capi, synthetic

    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true", help="skip the host yardsticks (they take minutes at 512^3)")
    ap.add_argument("--cpu-max-size", type=int, default=256, help="largest size the fast CPU labelling is timed on")
    ap.add_argument("--topology", action="store_true", help="time the component topology instead")
    ap.add_argument("--dists", nargs="+", default=["spheres"], help="--topology: the distributions to time")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(record):
        line = json.dumps(record)
        print(line, flush=True)
        lines.append(line)

    ctx = capi.Context(0)
    if args.topology:
        bench_topology(ctx, args, emit)
        ctx.close()
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return
    for size in args.sizes:
        shape = (size, size, size)
        vox = size ** 3
        for dist in ("spheres", "salt", "unknown_mix"):
            occ = synthetic.make_occupancy(shape, dist, seed=42)
            occ_dev = torch.from_numpy(occ).cuda()
            labels_dev = torch.empty(shape, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ms, count = [], 0
            for step in range(args.warmup + args.steps):
                ctx.synchronize()
                t0 = time.perf_counter()
                count = ctx.connected_components_dev(occ_dev.data_ptr(), shape, labels_dev.data_ptr())
                ctx.synchronize()
                if step >= args.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            rec = {"case": "connected_components_dev", "dist": dist, "shape": list(shape), "components": count}
            rec.update(_stats(ms))
            med = rec["median_ms"] * 1e-3
            rec["voxels_per_s"] = round(vox / med, 1)
            rec["floor"] = "%d B/voxel (4 occupancy read + 4 labels written) at %g GB/s" % (FLOOR_BYTES_PER_VOXEL,
                                                                                           HBM_PEAK_GBPS)
            rec["fraction_of_hbm_floor"] = round(FLOOR_BYTES_PER_VOXEL * vox / med / 1e9 / HBM_PEAK_GBPS, 4)
            if not args.no_cpu and size <= args.cpu_max_size:
                t0 = time.perf_counter()
                want, n = R.occupancy_labels_fast(occ)
                rec["cpu_fast_labels_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                rec["speedup_over_cpu_fast_labels"] = round(rec["cpu_fast_labels_ms"] / rec["median_ms"], 1)
                rec["equal_to_cpu"] = bool(n == count and
                                           np.array_equal(labels_dev.cpu().numpy().view(np.uint32), want))
            emit(rec)
            del occ_dev, labels_dev
    if not args.no_cpu:
        # the literal flood fill, at 128^3 only
        occ = synthetic.make_occupancy((128, 128, 128), "spheres", seed=42)
        t0 = time.perf_counter()
        want, n = R.occupancy_labels_flood(occ)
        flood_ms = (time.perf_counter() - t0) * 1e3
        ms = []
        for step in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            got, count = ctx.connected_components(occ)
            if step >= args.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        rec = {"case": "connected_components (host arrays)", "dist": "spheres", "shape": [128, 128, 128],
               "components": count, "cpu_flood_fill_ms": round(flood_ms, 1), "equal_to_cpu": bool(
                   n == count and np.array_equal(got, want))}
        rec.update(_stats(ms))
        rec["speedup_over_cpu_flood_fill"] = round(flood_ms / rec["median_ms"], 1)
        emit(rec)
    # the spatial-segment chain (SDF -> local extrema -> segments) on a tagged 256^3 scene, host labels out
    shape = (256, 256, 256)
    occ = synthetic.make_occupancy(shape, "unknown_mix", seed=42)
    coarse = np.random.default_rng(3).integers(0, 4, size=(8, 8, 8)).astype(np.uint32)
    ids = np.repeat(np.repeat(np.repeat(coarse, 32, 0), 32, 1), 32, 2) * (occ > 0.5)
    rec_cells = np.zeros(shape, dtype=capi.TAGGED_OBJECT_COMPONENT_CELL)
    rec_cells["occupancy"] = occ
    rec_cells["object_id"] = ids
    cells = ctx.cells(rec_cells, shape)
    res = 0.02
    ms, count = [], 0
    for step in range(args.warmup + args.steps):
        ctx.synchronize()
        t0 = time.perf_counter()
        _, count = cells.update_spatial_segments(1.75 * res, res)
        if step >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    rec = {"case": "cells_update_spatial_segments (labels to the host)", "shape": list(shape), "segments": count,
           "threshold": 1.75 * res, "resolution": res}
    rec.update(_stats(ms))
    rec["voxels_per_s"] = round(256 ** 3 / (rec["median_ms"] * 1e-3), 1)
    emit(rec)
    cells.close()
    ctx.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
