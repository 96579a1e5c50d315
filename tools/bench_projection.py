#!/usr/bin/env python3
"""Projection out of collision for a batch of points on a device-resident field: the one-kernel call beside the loop a
caller had to drive from the host before it existed.  One JSON line per clearance, and --out FILE for all of them.

  python tools/bench_projection.py [--size 256] [--queries 1000000] [--clearances 0 2] [--max-iterations 1000]
                                   [--steps 20] [--warmup 3] [--loop-steps 3] [--only-dev] [--out FILE]

  (a) vgt_hip_sdf_project_out_of_collision_dev, field and points on the device.
  (b) the host-driven loop: one vgt_hip_sdf_coarse_gradient_dev of the whole field (edge gradients on), then per step
      one vgt_hip_sdf_estimate_distance_dev of all the points and the gather of the cell's gradient, the norm, the step
      and the bookkeeping of the statuses as torch operations.  It runs as many steps as the slowest point of (a) took.
The field is the spheres scene at size^3 (0.01 per cell) extracted on the device; the points are uniform in the grid.
Both runs get the same explicit max_iterations (the library's default, 2 * 3 * size / 0.1 steps, would make the few
points that never get clear dominate (b) for minutes).  The results of (b) are compared with (a): statuses, and
positions to rounding (torch may contract a multiply-add that the kernel does not).

Timing: wall clock around the call with the stream drained before and after, `steps` repetitions after `warmup` (the
loop: `loop-steps` after one), median and min / max: the min-max range of one variant is the run-to-run spread that a
difference between two variants has to exceed.  --only-dev runs (a) alone: the form to put under
`rocprofv3 --kernel-trace --stats`, in a run of its own.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RESOLUTION = 0.01
MULTIPLIER = 0.1
BUCKETS = [0, 1, 11, 51, 101, 201, 501, 1001, 2001, 5001]   # lower edges of the iteration histogram


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


def _histogram(iterations):
    edges = BUCKETS + [np.iinfo(np.int32).max]
    counts = np.histogram(iterations, bins=edges)[0]
    labels = ["%d" % lo if hi - lo == 1 else "%d-%d" % (lo, hi - 1) for lo, hi in zip(edges[:-2], edges[1:-1])]
    labels.append(">=%d" % edges[-2])
    return {label: int(c) for label, c in zip(labels, counts)}


def host_driven_loop(ctx, torch, sdf, shape, queries, gradient, clearance, num_steps):
    """What a caller of the estimate and the coarse gradient had to do: every step is one estimate of all the points and a
    handful of torch kernels.  -> (position, status) as device tensors."""
    lib, n = ctx._lib, len(queries)
    nx, ny, nz = shape
    location = queries.clone()
    d = torch.empty(n, dtype=torch.float64, device="cuda")
    has = torch.empty(n, dtype=torch.uint8, device="cuda")
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    margin = clearance + RESOLUTION * MULTIPLIER * 1e-3
    max_step = RESOLUTION * MULTIPLIER

    def estimate():
        rc = lib.vgt_hip_sdf_estimate_distance_dev(ctx.handle, sdf.data_ptr(), nx, ny, nz, RESOLUTION, None,
                                                   location.data_ptr(), n, d.data_ptr(), has.data_ptr())
        assert rc == 0, rc

    estimate()
    status[has == 0] = 1
    live = (has != 0) & (d <= clearance)
    for _ in range(num_steps):
        cell = torch.floor(location * (1.0 / RESOLUTION)).to(torch.int64)
        linear = (cell[:, 0].clamp(0, nx - 1) * ny + cell[:, 1].clamp(0, ny - 1)) * nz + cell[:, 2].clamp(0, nz - 1)
        g = gradient[linear]
        norm = torch.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        flat = live & (norm <= RESOLUTION * 0.25)
        status[flat] = 2
        live = live & ~flat
        step = torch.minimum(margin - d, torch.full_like(d, max_step))
        moved = location + (g / norm[:, None]) * step[:, None]
        location = torch.where(live[:, None], moved, location)
        estimate()
        left = live & (has == 0)
        status[left] = 3
        live = live & (has != 0) & (d <= clearance)
    status[live] = 4
    location[status >= 2] = float("nan")
    return location, status


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--size", type=int, default=256)
    parser.add_argument("--queries", type=int, default=1_000_000)
    parser.add_argument("--clearances", type=float, nargs="+", default=[0.0, 2.0], help="in cells")
    parser.add_argument("--max-iterations", type=int, default=1000)
    parser.add_argument("--steps", type=int, default=20)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--loop-steps", type=int, default=3)
    parser.add_argument("--only-dev", action="store_true")
    parser.add_argument("--out")
    args = parser.parse_args()

    import torch
    from voxelized_geometry_tools_amd import capi, synthetic
    if not torch.cuda.is_available():
        sys.exit("bench_projection.py needs a HIP device (no CPU fallback)")
    shape = (args.size,) * 3
    ctx = capi.Context(0)
    ctx.set_stream(None)   # the stream torch works on: the loop interleaves the library's kernels with torch's
    occ = torch.from_numpy(synthetic.make_occupancy(shape, "spheres", seed=42)).cuda()
    sdf = torch.empty(shape, dtype=torch.float32, device="cuda")
    nbytes = capi.sdf_workspace_bytes(shape)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ctx.sdf_dev(occ.data_ptr(), shape, RESOLUTION, sdf.data_ptr(), workspace.data_ptr(), nbytes)
    ctx.synchronize()
    del workspace, occ
    n = args.queries
    queries = torch.from_numpy(np.random.default_rng(7).random((n, 3)) * (args.size * RESOLUTION)).cuda()
    position = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    has = torch.empty(n, dtype=torch.uint8, device="cuda")
    status = torch.empty(n, dtype=torch.uint8, device="cuda")
    iterations = torch.empty(n, dtype=torch.int32, device="cuda")
    gradient = None
    results = []
    for cells in args.clearances:
        clearance = cells * RESOLUTION

        def one_kernel():
            ctx.sdf_project_out_of_collision_dev(sdf.data_ptr(), shape, RESOLUTION, queries.data_ptr(), n,
                                                 position.data_ptr(), has.data_ptr(), status.data_ptr(),
                                                 iterations.data_ptr(), minimum_distance=clearance,
                                                 stepsize_multiplier=MULTIPLIER, max_iterations=args.max_iterations)

        dev_ms, _ = _timed(ctx, one_kernel, args.warmup, args.steps)
        steps_taken = iterations.cpu().numpy()
        dev_status = status.cpu().numpy()
        record = {"bench": "projection", "size": args.size, "queries": n, "clearance_cells": cells,
                  "stepsize_multiplier": MULTIPLIER, "max_iterations": args.max_iterations,
                  "one_kernel": _stats(dev_ms), "statuses": np.bincount(dev_status, minlength=5).tolist(),
                  "iterations_total": int(steps_taken.sum()), "iterations_max": int(steps_taken.max()),
                  "iterations_histogram": _histogram(steps_taken)}
        record["one_kernel"]["ns_per_step"] = round(record["one_kernel"]["median_ms"] * 1e6 /
                                                    max(1, record["iterations_total"]), 3)
        if not args.only_dev:
            if gradient is None:
                gradient = torch.empty((args.size ** 3, 3), dtype=torch.float64, device="cuda")
                gradient_ms, _ = _timed(ctx, lambda: capi.check(ctx._lib.vgt_hip_sdf_coarse_gradient_dev(
                    ctx.handle, sdf.data_ptr(), *shape, RESOLUTION, 1, None, gradient.data_ptr(), None)), 1, 3)
            num_steps = int(steps_taken.max())
            loop_ms, (loop_position, loop_status) = _timed(
                ctx, lambda: host_driven_loop(ctx, torch, sdf, shape, queries, gradient, clearance, num_steps), 1,
                args.loop_steps)
            loop_status = loop_status.cpu().numpy()
            same = loop_status == dev_status
            valued = same & (dev_status == 0)
            difference = (loop_position.cpu().numpy()[valued] - position.cpu().numpy()[valued])
            record.update({"host_driven_loop": _stats(loop_ms), "host_driven_loop_steps": num_steps,
                           "whole_field_gradient": _stats(gradient_ms),
                           "statuses_equal": int(same.sum()), "max_position_difference":
                           float(np.abs(difference).max(initial=0.0)),
                           "speedup": round(float(np.median(loop_ms) / np.median(dev_ms)), 1)})
        results.append(record)
        print(json.dumps(record), flush=True)
    ctx.reset_stream()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
