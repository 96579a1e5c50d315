#!/usr/bin/env python3
"""Sphere-model checks (vgt_hip_check_spheres_dev) on device-resident fields, models and poses, beside what a caller could
do before the call existed.  One JSON line per measurement, and --out FILE (default profiles/bodies/bench_bodies.json)
for all of them.

  python tools/bench_bodies.py [--sizes 256 512] [--configurations 10000 100000 1000000] [--spheres 16 64 200]
                               [--links 8] [--steps 10] [--warmup 3] [--label TEXT] [--out FILE]

The field is the SDF of the spheres scene (D1) at size^3, 0.01 per cell, extracted on the device.  A model has S spheres
of radius 0 - 0.03 within 0.1 of the origins of L links; a configuration places every link uniformly in the grid's box
with a uniform random rotation.  Per (size, B, S), three things are timed:

  check            vgt_hip_check_spheres_dev, per-configuration outputs only
  check+spheres    the same with sphere_clearance and sphere_gradient
  yardstick        what a caller can do without the call: vgt_hip_sdf_estimate_distance_dev on the B * S centres --
                   ALREADY transformed and resident, so the transform is not charged to it --, then a torch subtraction
                   of the radii and torch.min over [B, S] (values and indices in one reduction)

and the record gives both times and their ratio (yardstick / check: above 1, the call is faster).  The tool also checks
that the yardstick's minima equal the call's min_clearance where both are finite (they evaluate the same estimate).

floor_share: the time the per-configuration traffic alone would take at the HBM's 8 TB/s, over the time measured.  The
floor is a CONVENTION -- L * 96 bytes of poses read plus the outputs written (45 bytes per configuration; with the
per-sphere outputs 32 more per sphere) -- because what the gathers of the field cost depends on how much of it the caches
hold, which no formula over shapes knows.

Timing: wall clock around the enqueue and a synchronise of the stream (drained before, too), `steps` repetitions after
`warmup`, median and min / max: the min - max range of one variant is the run-to-run spread a difference has to exceed.
--label names the build in the records (the A/B of the pose staging runs this tool once per build, alternating, with
VGT_HIP_LIB pointing at the build).
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
MINIMUM_CLEARANCE = 0.02
HBM_BYTES_PER_S = 8.0e12


def _stats(ms):
    ms = np.asarray(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4),
            "max_ms": round(float(ms.max()), 4), "steps": int(ms.size)}


def _timed(ctx, call, warmup, steps):
    ms = []
    for step in range(warmup + steps):
        ctx.synchronize()
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        if step >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def scene_sdf(ctx, torch, capi, synthetic, size):
    shape = (size,) * 3
    occ = torch.from_numpy(synthetic.make_occupancy(shape, "spheres", seed=42)).cuda()
    sdf = torch.empty(shape, dtype=torch.float32, device="cuda")
    nbytes = capi.sdf_workspace_bytes(shape)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ctx.sdf_dev(occ.data_ptr(), shape, RESOLUTION, sdf.data_ptr(), workspace.data_ptr(), nbytes)
    ctx.synchronize()
    return sdf


def make_model(torch, num_spheres, num_links, seed):
    rng = np.random.default_rng(seed)
    xyzr = np.empty((num_spheres, 4))
    xyzr[:, :3] = (rng.random((num_spheres, 3)) - 0.5) * 0.2
    xyzr[:, 3] = rng.random(num_spheres) * 0.03
    link = rng.integers(0, num_links, num_spheres).astype(np.int32)
    return torch.from_numpy(xyzr).cuda(), torch.from_numpy(link).cuda()


def make_poses(torch, num_configurations, num_links, extent, seed):
    """[B, L, 16] column-major, generated on the device: uniform rotations (normalised Gaussian quaternions), translations
    uniform in the grid's box."""
    generator = torch.Generator(device="cuda")
    generator.manual_seed(seed)
    q = torch.randn((num_configurations, num_links, 4), dtype=torch.float64, device="cuda", generator=generator)
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    t = torch.rand((num_configurations, num_links, 3), dtype=torch.float64, device="cuda", generator=generator) * extent
    zero, one = torch.zeros_like(w), torch.ones_like(w)
    columns = [1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w), zero,
               2 * (x * y - z * w), 1 - 2 * (x * x + z * z), 2 * (y * z + x * w), zero,
               2 * (x * z + y * w), 2 * (y * z - x * w), 1 - 2 * (x * x + y * y), zero,
               t[..., 0], t[..., 1], t[..., 2], one]
    return torch.stack(columns, dim=-1).contiguous()


def world_centres(torch, xyzr, link, poses):
    """[B, S, 3] contiguous, for the yardstick (its own arithmetic: the yardstick is a timing, not a parity test)"""
    b, s = poses.shape[0], xyzr.shape[0]
    x, y, z = xyzr[:, 0], xyzr[:, 1], xyzr[:, 2]
    centres = torch.empty((b, s, 3), dtype=torch.float64, device="cuda")
    chunk = max(1, 4_000_000 // s)                                                  # (the gathered poses: 128 B per pair)
    for first in range(0, b, chunk):
        m = poses[first:first + chunk][:, link.long(), :]                           # [chunk, S, 16]
        for r in range(3):
            centres[first:first + chunk, :, r] = ((m[..., r] * x + m[..., 4 + r] * y) + m[..., 8 + r] * z) + m[..., 12 + r]
    return centres


def one_shape(ctx, torch, sdf, size, b, s, links, args):
    shape = (size,) * 3
    xyzr, link = make_model(torch, s, links, 1000 + s)
    poses = make_poses(torch, b, links, size * RESOLUTION, 2000 + s)
    out = {"status": torch.empty(b, dtype=torch.uint8, device="cuda"),
           "min_clearance": torch.empty(b, dtype=torch.float64, device="cuda"),
           "min_sphere": torch.empty(b, dtype=torch.int32, device="cuda"),
           "num_below": torch.empty(b, dtype=torch.int32, device="cuda"),
           "num_outside": torch.empty(b, dtype=torch.int32, device="cuda"),
           "min_gradient": torch.empty((b, 3), dtype=torch.float64, device="cuda")}
    per_sphere = {"sphere_clearance": torch.empty((b, s), dtype=torch.float64, device="cuda"),
                  "sphere_gradient": torch.empty((b, s, 3), dtype=torch.float64, device="cuda")}

    def check(extra):
        ctx.check_spheres_dev(sdf.data_ptr(), shape, RESOLUTION, xyzr.data_ptr(), link.data_ptr(), s, poses.data_ptr(),
                              links, b, out["status"].data_ptr(),
                              **{name + "_ptr": t.data_ptr() for name, t in out.items() if name != "status"},
                              **{name + "_ptr": t.data_ptr() for name, t in extra.items()},
                              minimum_clearance=MINIMUM_CLEARANCE)

    check_ms = _timed(ctx, lambda: check({}), args.warmup, args.steps)
    spheres_ms = _timed(ctx, lambda: check(per_sphere), args.warmup, args.steps)
    min_clearance = out["min_clearance"].clone()
    statuses = np.bincount(out["status"].cpu().numpy(), minlength=3).tolist()
    del per_sphere

    centres = world_centres(torch, xyzr, link, poses)
    distance = torch.empty(b * s, dtype=torch.float64, device="cuda")
    radius = xyzr[:, 3].contiguous()
    result = {}

    def yardstick():
        ctx.sdf_estimate_distance_dev(sdf.data_ptr(), shape, RESOLUTION, centres.data_ptr(), b * s, distance.data_ptr())
        clearance = distance.view(b, s) - radius
        result["min"] = clearance.min(dim=1)

    yardstick_ms = _timed(ctx, yardstick, args.warmup, args.steps)
    both = torch.isfinite(result["min"].values) & torch.isfinite(min_clearance)
    # (where a configuration has a sphere outside the grid the yardstick's minimum is NaN: compared where both have one)
    same = bool(torch.equal(result["min"].values[both], min_clearance[both]))

    record = {"bench": "bodies", "label": args.label, "scene": "spheres", "size": size, "configurations": b, "spheres": s,
              "links": links, "minimum_clearance": MINIMUM_CLEARANCE, "statuses_clear_collision_novalue": statuses,
              "check": _stats(check_ms), "check_with_spheres": _stats(spheres_ms), "yardstick": _stats(yardstick_ms),
              "yardstick_minima_equal": same, "compared_configurations": int(both.sum().item())}
    record["yardstick_over_check"] = round(record["yardstick"]["median_ms"] / record["check"]["median_ms"], 3)
    record["yardstick_over_check_with_spheres"] = round(
        record["yardstick"]["median_ms"] / record["check_with_spheres"]["median_ms"], 3)
    floor = b * (links * 96 + 45)
    floor_spheres = floor + b * s * 32
    record["floor_bytes"] = floor
    record["floor_share"] = round(floor / HBM_BYTES_PER_S / (record["check"]["median_ms"] * 1e-3), 4)
    record["floor_bytes_with_spheres"] = floor_spheres
    record["floor_share_with_spheres"] = round(
        floor_spheres / HBM_BYTES_PER_S / (record["check_with_spheres"]["median_ms"] * 1e-3), 4)
    record["pairs_per_s"] = round(b * s / (record["check"]["median_ms"] * 1e-3))
    print(json.dumps(record), flush=True)
    return record


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    parser.add_argument("--configurations", type=int, nargs="+", default=[10_000, 100_000, 1_000_000])
    parser.add_argument("--spheres", type=int, nargs="+", default=[16, 64, 200])
    parser.add_argument("--links", type=int, default=8)
    parser.add_argument("--steps", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--label", default="")
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "bodies", "bench_bodies.json"))
    args = parser.parse_args()

    import torch
    from voxelized_geometry_tools_amd import capi, synthetic
    if not torch.cuda.is_available():
        sys.exit("bench_bodies.py needs a HIP device (no CPU fallback)")
    ctx = capi.Context(0)
    ctx.set_stream(None)   # the stream torch works on
    results = []
    for size in args.sizes:
        sdf = scene_sdf(ctx, torch, capi, synthetic, size)
        for b in args.configurations:
            for s in args.spheres:
                results.append(one_shape(ctx, torch, sdf, size, b, s, args.links, args))
                torch.cuda.empty_cache()
        del sdf
    ctx.reset_stream()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
