#!/usr/bin/env python3
"""Sphere models into voxel grids (vgt_hip_rasterize_spheres_dev) and onto point clouds
(vgt_hip_spheres_cover_points_dev), device-resident, beside what a caller could do before the calls existed.  One JSON line
per measurement, and --out FILE (default profiles/volumes/bench_volumes.json) for all of them.

  python tools/bench_volumes.py [--sizes 256 512] [--configurations 100 10000] [--spheres 16 64 200] [--links 8]
                                [--points 1000000] [--point-configurations 1 64] [--steps 20] [--warmup 3]
                                [--yardstick-steps 20] [--out FILE]

Grid form.  size^3 cells at 0.01.  A model has S spheres of radius 0.02 - 0.05 (2 to 5 cells) within 0.08 of the origins
of L links; the B configurations lie along a straight motion -- the swept-volume case: every link's origin moves on a
straight line across the grid while the link turns by a quarter turn about a fixed axis.  Timed: the call (its fill to -1
included).  Counted, in ONE extra run of the testing library's counting kernel
(vgt_hip_testing_set_sphere_volume_counters): the (cell, sphere) tests the launch made (the cells of every box), those
that covered, and the atomics issued; tests_per_s is the count over the product kernel's median time, and
atomic_share = atomics / covering tests.  A counting build, not a derivation from first_configuration: the output says
which cells were lowered at least once, not how often.

Point form.  N points, half of them within 0.06 of sphere centres of random configurations, half uniform in the box;
the same models and motion.  tests_per_s counts the (point, sphere) tests the scan rule makes -- b * S + s + 1 for a
point first covered by (b, s), B * S for an uncovered one, derived from the outputs -- over the median time.

Yardstick: the torch broadcast over ALREADY transformed centres that a caller could write at the parent commit, per
configuration b: d2 = ((q[:, None, :] - c[b][None, :, :]) ** 2).sum(-1) <= R ** 2, any over the spheres, and the first b
kept per cell or point.  It holds cells x S x 3 doubles several times over, so it runs where three such arrays fit
--yardstick-bytes (default 96 GiB) and for at most --yardstick-configurations configurations (default 100; its time is
linear in B and is reported as measured, for that B, beside the call's time for the same configurations; measured once
per (size, S), with the first --configurations value);
--yardstick-steps repetitions after `warmup`.  The record states both times and their ratio, and how many answers differ
(the yardstick sums in torch's order, so cells on a rounding tie may differ; that is reported, not asserted).

Timing: wall clock around the enqueue and a synchronise of the stream (drained before, too), `steps` repetitions after
`warmup`, median and min / max of the same run.
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


def _stats(ms):
    ms = np.asarray(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4),
            "max_ms": round(float(ms.max()), 4), "steps": int(ms.size)}


def _timed(sync, call, warmup, steps):
    ms = []
    for step in range(warmup + steps):
        sync()
        t0 = time.perf_counter()
        call()
        sync()
        if step >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def make_model(torch, num_spheres, num_links, seed):
    rng = np.random.default_rng(seed)
    xyzr = np.empty((num_spheres, 4))
    xyzr[:, :3] = (rng.random((num_spheres, 3)) - 0.5) * 0.16
    xyzr[:, 3] = 0.02 + rng.random(num_spheres) * 0.03
    link = rng.integers(0, num_links, num_spheres).astype(np.int32)
    return torch.from_numpy(xyzr).cuda(), torch.from_numpy(link).cuda()


def make_motion(torch, num_configurations, num_links, extent, seed):
    """[B, L, 16] column-major: link k moves from start_k to end_k on a straight line and turns a quarter turn about axis_k."""
    rng = np.random.default_rng(seed)
    start = (0.15 + rng.random((num_links, 3)) * 0.2) * extent
    end = (0.65 + rng.random((num_links, 3)) * 0.2) * extent
    axis = rng.normal(size=(num_links, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    t = torch.linspace(0.0, 1.0, num_configurations, dtype=torch.float64, device="cuda")[:, None]      # [B, 1]
    half = t * (np.pi / 4)                                                                              # half the angle
    ax = torch.from_numpy(axis).cuda()                                                                  # [L, 3]
    w = torch.cos(half).expand(-1, num_links)
    x, y, z = (torch.sin(half) * ax[None, :, k] for k in range(3))
    p = torch.from_numpy(start).cuda()[None] * (1.0 - t[:, :, None]) + torch.from_numpy(end).cuda()[None] * t[:, :, None]
    zero, one = torch.zeros_like(w), torch.ones_like(w)
    columns = [1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w), zero,
               2 * (x * y - z * w), 1 - 2 * (x * x + z * z), 2 * (y * z + x * w), zero,
               2 * (x * z + y * w), 2 * (y * z - x * w), 1 - 2 * (x * x + y * y), zero,
               p[..., 0], p[..., 1], p[..., 2], one]
    return torch.stack(columns, dim=-1).contiguous()


def world_centres(torch, xyzr, link, poses):
    """[B, S, 3] (the yardstick's input: already transformed, not charged to it)"""
    x, y, z = xyzr[:, 0], xyzr[:, 1], xyzr[:, 2]
    m = poses[:, link.long(), :]
    return torch.stack([((m[..., r] * x + m[..., 4 + r] * y) + m[..., 8 + r] * z) + m[..., 12 + r] for r in range(3)],
                       dim=-1).contiguous()


def broadcast_first(torch, q, centres, radius, num_configurations):
    """The yardstick: q [M, 3] against centres [B, S, 3], first covering b per row of q (int32, -1 without one)."""
    first = torch.full((q.shape[0],), -1, dtype=torch.int32, device="cuda")
    rr = radius * radius
    for b in range(num_configurations):
        covered = ((((q[:, None, :] - centres[b][None, :, :]) ** 2).sum(-1)) <= rr).any(dim=1)
        first = torch.where((first < 0) & covered, torch.full_like(first, b), first)
    return first


def grid_shape(ctx, testing, torch, size, b, s, links, args, with_yardstick):
    shape = (size,) * 3
    xyzr, link = make_model(torch, s, links, 1000 + s)
    poses = make_motion(torch, b, links, size * RESOLUTION, 2000 + s)
    first = torch.empty(shape, dtype=torch.int32, device="cuda")

    def call(c=ctx):
        c.rasterize_spheres_dev(shape, RESOLUTION, xyzr.data_ptr(), link.data_ptr(), s, poses.data_ptr(), links, b,
                                first.data_ptr())

    ms = _timed(ctx.synchronize, call, args.warmup, args.steps)
    answer = first.clone()
    counters = torch.zeros(3, dtype=torch.int64, device="cuda")
    testing.set_sphere_volume_counters(counters.data_ptr())
    try:
        call(testing)
        testing.synchronize()
    finally:
        testing.set_sphere_volume_counters(None)
    tests, covering, atomics = (int(v) for v in counters.cpu().numpy())
    record = {"bench": "volumes", "form": "grid", "size": size, "configurations": b, "spheres": s, "links": links,
              "rasterize": _stats(ms), "covered_cells": int((answer >= 0).sum().item()),
              "counting_run_equal": bool(torch.equal(first, answer)), "tests": tests, "covering_tests": covering,
              "atomics": atomics, "atomic_share": round(atomics / covering, 5) if covering else None,
              "counts_from": "one run of the testing library's counting kernel"}
    record["tests_per_s"] = round(tests / (record["rasterize"]["median_ms"] * 1e-3))
    yb = min(b, args.yardstick_configurations)
    if not with_yardstick:
        record["yardstick"] = "not run: measured once per (size, spheres), with the first --configurations value"
    elif size ** 3 * s * 3 * 8 * 3 <= args.yardstick_bytes:                      # (the difference, its square, slack)
        centres = world_centres(torch, xyzr, link, poses[:yb])
        axes = (torch.arange(size, dtype=torch.float64, device="cuda") + 0.5) * RESOLUTION
        q = torch.stack(torch.meshgrid(axes, axes, axes, indexing="ij"), dim=-1).reshape(-1, 3)
        result = {}

        def yardstick():
            result["first"] = broadcast_first(torch, q, centres, xyzr[:, 3], yb)

        try:
            yms = _timed(torch.cuda.synchronize, yardstick, args.warmup, args.yardstick_steps)
        except torch.OutOfMemoryError:
            yms = None
        part = torch.empty(shape, dtype=torch.int32, device="cuda")
        pms = _timed(ctx.synchronize, lambda: ctx.rasterize_spheres_dev(
            shape, RESOLUTION, xyzr.data_ptr(), link.data_ptr(), s, poses.data_ptr(), links, yb, part.data_ptr()),
            args.warmup, args.steps)
        if yms is None:
            record["yardstick"] = "not run: out of device memory"
        else:
            record["yardstick"] = dict(_stats(yms), configurations=yb, rasterize_same_configurations=_stats(pms),
                                       cells_differing=int((result["first"] != part.reshape(-1)).sum().item()))
            record["yardstick_over_rasterize"] = round(
                record["yardstick"]["median_ms"] / record["yardstick"]["rasterize_same_configurations"]["median_ms"], 1)
        del q, centres, result
    else:
        record["yardstick"] = "not run: cells x S x 3 doubles do not fit --yardstick-bytes"
    print(json.dumps(record), flush=True)
    return record


def point_shape(ctx, torch, n, b, s, links, args):
    extent = 256 * RESOLUTION
    xyzr, link = make_model(torch, s, links, 1000 + s)
    poses = make_motion(torch, b, links, extent, 2000 + s)
    centres = world_centres(torch, xyzr, link, poses)
    generator = torch.Generator(device="cuda")
    generator.manual_seed(5)
    points = torch.rand((n, 3), dtype=torch.float64, device="cuda", generator=generator) * extent
    pick_b = torch.randint(0, b, (n // 2,), device="cuda", generator=generator)
    pick_s = torch.randint(0, s, (n // 2,), device="cuda", generator=generator)
    points[:n // 2] = centres[pick_b, pick_s] + (torch.rand((n // 2, 3), dtype=torch.float64, device="cuda",
                                                            generator=generator) - 0.5) * 0.12
    points = points[torch.randperm(n, device="cuda", generator=generator)].float().contiguous()
    first_b = torch.empty(n, dtype=torch.int32, device="cuda")
    first_s = torch.empty(n, dtype=torch.int32, device="cuda")
    filtered = torch.empty((n, 3), dtype=torch.float32, device="cuda")

    def call():
        ctx.spheres_cover_points_dev(points.data_ptr(), n, xyzr.data_ptr(), link.data_ptr(), s, poses.data_ptr(), links, b,
                                     first_b.data_ptr(), first_s.data_ptr(), filtered.data_ptr())

    ms = _timed(ctx.synchronize, call, args.warmup, args.steps)
    found = first_b >= 0
    tests = int(torch.where(found, first_b.long() * s + first_s.long() + 1, torch.full_like(first_b, b * s).long()).sum().item())
    record = {"bench": "volumes", "form": "points", "points": n, "configurations": b, "spheres": s, "links": links,
              "cover": _stats(ms), "covered_points": int(found.sum().item()), "tests": tests, "tests_if_none_covered": n * b * s}
    record["tests_per_s"] = round(tests / (record["cover"]["median_ms"] * 1e-3))
    q = points.double()
    result = {}

    def yardstick():
        result["first"] = broadcast_first(torch, q, centres, xyzr[:, 3], b)

    yms = _timed(torch.cuda.synchronize, yardstick, args.warmup, args.yardstick_steps)
    record["yardstick"] = dict(_stats(yms), points_differing=int((result["first"] != first_b).sum().item()))
    record["yardstick_over_cover"] = round(record["yardstick"]["median_ms"] / record["cover"]["median_ms"], 1)
    print(json.dumps(record), flush=True)
    return record


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--sizes", type=int, nargs="*", default=[256, 512])
    parser.add_argument("--configurations", type=int, nargs="+", default=[100, 10_000])
    parser.add_argument("--spheres", type=int, nargs="+", default=[16, 64, 200])
    parser.add_argument("--links", type=int, default=8)
    parser.add_argument("--points", type=int, default=1_000_000)
    parser.add_argument("--point-configurations", type=int, nargs="*", default=[1, 64])
    parser.add_argument("--steps", type=int, default=20)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--yardstick-steps", type=int, default=20)
    parser.add_argument("--yardstick-configurations", type=int, default=100)
    parser.add_argument("--yardstick-bytes", type=int, default=96 << 30)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "volumes", "bench_volumes.json"))
    args = parser.parse_args()

    import torch
    from voxelized_geometry_tools_amd import capi
    if not torch.cuda.is_available():
        sys.exit("bench_volumes.py needs a HIP device (no CPU fallback)")
    ctx = capi.Context(0)
    ctx.set_stream(None)   # the stream torch works on
    testing = capi.Context(0, testing=True)
    testing.set_stream(None)
    results = [{"bench": "volumes", "device": torch.cuda.get_device_name(0), "resolution": RESOLUTION,
                "steps": args.steps, "warmup": args.warmup}]
    for size in args.sizes:
        for b in args.configurations:
            for s in args.spheres:
                results.append(grid_shape(ctx, testing, torch, size, b, s, args.links, args, b == args.configurations[0]))
                torch.cuda.empty_cache()
    for b in args.point_configurations:
        for s in args.spheres:
            results.append(point_shape(ctx, torch, args.points, b, s, args.links, args))
            torch.cuda.empty_cache()
    for c in (testing, ctx):
        c.reset_stream()
        c.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
