#!/usr/bin/env python3
"""Cloud alignment (vgt_hip_align_points_dev) on device-resident fields, clouds and poses, beside what a caller could do
before the call existed.  One JSON line per measurement, and --out FILE (default profiles/align/bench_align.json) for all
of them.

  python tools/bench_align.py [--sizes 256 512] [--cases 1x100000x10 1x1000000x10 10000x10000x0] [--steps 10]
                              [--warmup 3] [--out FILE]

The field is the SDF of the spheres scene (D1) at size^3, 0.01 per cell, extracted on the device.  The cloud is N points
drawn from the cells within one cell of a surface, jittered inside their cells and moved into a sensor frame by the
inverse of a known pose; the B hypotheses are that pose moved by up to 2 cells and 2 degrees about the grid's centre.  A
case is B x N x K.  Per (size, case), measured in ONE process and interleaved (align, baseline, align, baseline ...):

  align       vgt_hip_align_points_dev with K steps and tolerances of 0, so that every pose takes its K steps
  score       the same call with K = 0: one evaluation and its bookkeeping
  baseline    the route without the call, once: a torch transform of the N points by the B poses (float64), then
              vgt_hip_sdf_estimate_distance_dev on the B * N centres, then a torch sum of squares per pose over the
              centres with a value.  It has no Jacobian and takes no step: K + 1 of it is a LOWER bound on what a K-step
              refinement costs that way.
  estimate    vgt_hip_sdf_estimate_distance_dev alone on the B * N centres, already transformed and resident: the
              kernel whose gathers the evaluation repeats

and the record gives the medians with their min - max (the run-to-run spread a difference has to exceed), the time per
iteration ((align - score) / K), score / estimate, and align / ((K + 1) * baseline).  The tool checks that the score's
sum of squares equals the baseline's to 1e-9 relative (the same estimates, summed in another order).

Timing: wall clock around the enqueue and a synchronise of the stream (drained before, too), `steps` repetitions after
`warmup`.  The split across the kernels comes from a run of its own under rocprofv3 --kernel-trace --stats.
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


def _interleaved(ctx, calls, warmup, steps):
    """{name: [ms]}: the calls one after the other, round after round"""
    ms = {name: [] for name in calls}
    for step in range(warmup + steps):
        for name, call in calls.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            call()
            ctx.synchronize()
            if step >= warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
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


def rotation(axis, degrees):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    a = np.radians(degrees)
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def matrix(R, t):
    m = np.eye(4)
    m[:3, :3] = R
    m[:3, 3] = t
    return m


def make_inputs(torch, sdf, size, num_points, num_poses, seed):
    """(points [N, 3] float32 on the device, poses [B, 16] float64 on the device, the grid's centre)"""
    rng = np.random.default_rng(seed)
    near = torch.nonzero(sdf.abs() <= RESOLUTION)                                   # cells next to a surface
    pick = torch.from_numpy(rng.integers(0, len(near), num_points)).cuda()
    world = (near[pick].double() + torch.from_numpy(rng.random((num_points, 3))).cuda()) * RESOLUTION
    centre = np.full(3, size * RESOLUTION * 0.5)
    truth = matrix(rotation([0.3, -0.5, 0.8], 25.0), [0.31, 0.52, -0.17])
    inverse = torch.from_numpy(np.linalg.inv(truth)).cuda()
    points = (world @ inverse[:3, :3].T + inverse[:3, 3]).float().contiguous()
    poses = np.empty((num_poses, 16))
    for b in range(num_poses):
        R = rotation(rng.normal(size=3), 2.0 * rng.random())
        shift = (rng.random(3) - 0.5) * 4.0 * RESOLUTION
        poses[b] = (matrix(R, centre - R @ centre + shift) @ truth).T.reshape(16)
    return points, torch.from_numpy(poses).cuda(), centre


def one_case(ctx, torch, capi, sdf, size, b, n, k, args):
    shape = (size,) * 3
    points, poses, centre = make_inputs(torch, sdf, size, n, b, 7 * size + n % 1000 + b)
    size_bytes = capi.align_points_workspace_bytes(n, b)
    workspace = torch.empty(size_bytes, dtype=torch.uint8, device="cuda")
    out = {"poses_out": torch.empty((b, 16), dtype=torch.float64, device="cuda"),
           "status": torch.empty(b, dtype=torch.uint8, device="cuda"),
           "num_used": torch.empty(b, dtype=torch.int32, device="cuda"),
           "sum_squared": torch.empty(b, dtype=torch.float64, device="cuda"),
           "evaluations": torch.empty(b, dtype=torch.int32, device="cuda")}
    target = -0.5 * RESOLUTION

    def align(steps):
        ctx.align_points_dev(sdf.data_ptr(), shape, RESOLUTION, points.data_ptr(), n, poses.data_ptr(), b,
                             out["status"].data_ptr(), workspace.data_ptr(), size_bytes,
                             **{name + "_ptr": t.data_ptr() for name, t in out.items() if name != "status"},
                             max_iterations=steps, damping=1e-3, target_distance=target, pivot=centre)

    distance = torch.empty(b * n, dtype=torch.float64, device="cuda")
    has = torch.empty(b * n, dtype=torch.uint8, device="cuda")
    rot = poses.view(b, 4, 4)[:, :3, :3]                                            # (column-major: [b, column, row])
    shift = poses.view(b, 4, 4)[:, 3, :3]
    result = {}

    def transform():
        return (torch.matmul(points.double().unsqueeze(0), rot) + shift.unsqueeze(1)).contiguous()

    def baseline():
        centres = transform()
        ctx.sdf_estimate_distance_dev(sdf.data_ptr(), shape, RESOLUTION, centres.data_ptr(), b * n, distance.data_ptr(),
                                      has.data_ptr())
        r = torch.where(has.view(b, n) != 0, distance.view(b, n) - target, torch.zeros((), dtype=torch.float64,
                                                                                       device="cuda"))
        result["sum"] = (r * r).sum(dim=1)

    fixed = transform()

    def estimate():
        ctx.sdf_estimate_distance_dev(sdf.data_ptr(), shape, RESOLUTION, fixed.data_ptr(), b * n, distance.data_ptr(),
                                      has.data_ptr())

    calls = {"score": lambda: align(0), "baseline": baseline, "estimate": estimate}
    if k > 0:
        calls["align"] = lambda: align(k)
    ms = _interleaved(ctx, calls, args.warmup, args.steps)
    align(0)
    baseline()
    ctx.synchronize()
    scored = out["sum_squared"].clone()
    close = bool(torch.allclose(scored, result["sum"], rtol=1e-9, atol=0.0))
    record = {"bench": "align", "scene": "spheres", "size": size, "poses": b, "points": n, "max_iterations": k,
              "score": _stats(ms["score"]), "baseline": _stats(ms["baseline"]), "estimate": _stats(ms["estimate"]),
              "score_sum_equals_baseline": close,
              "used_share": round(float(out["num_used"].double().mean().item()) / n, 4)}
    record["score_over_estimate"] = round(record["score"]["median_ms"] / record["estimate"]["median_ms"], 3)
    record["score_over_baseline"] = round(record["score"]["median_ms"] / record["baseline"]["median_ms"], 3)
    record["pairs_per_s_score"] = round(b * n / (record["score"]["median_ms"] * 1e-3))
    if k > 0:
        align(k)
        ctx.synchronize()
        record["align"] = _stats(ms["align"])
        record["evaluations"] = np.bincount(out["evaluations"].cpu().numpy()).tolist()
        record["statuses"] = np.bincount(out["status"].cpu().numpy(), minlength=4).tolist()
        record["per_iteration_ms"] = round((record["align"]["median_ms"] - record["score"]["median_ms"]) / k, 4)
        record["align_over_k_plus_1_baselines"] = round(
            record["align"]["median_ms"] / ((k + 1) * record["baseline"]["median_ms"]), 3)
    print(json.dumps(record), flush=True)
    return record


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    parser.add_argument("--cases", nargs="+", default=["1x100000x10", "1x1000000x10", "10000x10000x0"],
                        help="poses x points x steps")
    parser.add_argument("--steps", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "align", "bench_align.json"))
    args = parser.parse_args()
    cases = [tuple(int(v) for v in case.split("x")) for case in args.cases]

    import torch
    from voxelized_geometry_tools_amd import capi, synthetic
    if not torch.cuda.is_available():
        sys.exit("bench_align.py needs a HIP device (no CPU fallback)")
    ctx = capi.Context(0)
    ctx.set_stream(None)   # the stream torch works on
    results = []
    for size in args.sizes:
        sdf = scene_sdf(ctx, torch, capi, synthetic, size)
        for b, n, k in cases:
            results.append(one_case(ctx, torch, capi, sdf, size, b, n, k, args))
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
