#!/usr/bin/env python3
"""Inverse kinematics (vgt_hip_solve_ik_dev) on device-resident targets and seeds, beside the only route there was before
the call existed.  One JSON line per measurement, and --out FILE (default profiles/ik/bench_ik.json) for all of them.

  python tools/bench_ik.py [--problems 10000 100000 1000000] [--spreads 0.1 1.0] [--iterations 20 100]
                           [--seeds-per-target 4] [--steps 5] [--warmup 2] [--draws 2] [--out FILE]

Two trees (tools/bench_kinematics.py's): `arm`, a serial arm of 8 links with the tool as the tip (seven revolute joints on
the chain), and `body`, 15 links, with the right hand's tool frame as the tip (a lift and three revolute joints on the
chain, six columns off it).  Targets are the forward kinematics of rows drawn in +-2.5 (the lift and the grippers:
+-0.1); the seeds are the truth plus a uniform perturbation of +- spread; lambda = 0.01, max_step 0.5, tolerances 1e-6,
no limits.  Per (tree, B, spread, K) and draw:

  ik               vgt_hip_solve_ik_dev, every output
  torch            the route a caller had: a host-side loop over iterations, each with vgt_hip_forward_kinematics_dev for
                   the poses and batched torch in float64 for the error, the columns, A, torch.linalg.solve and the
                   update, on all B rows with the stopped ones masked, until no row is live (one device-to-host flag per
                   iteration).  Its own arithmetic: a timing, not a parity test
  agreement        before anything is timed: the statuses of the two must be equal on every row, and the joints within
                   1e-9 on every row that converged.  (A row that never converges wanders for K steps under a clipped
                   step, where the last bits of the two solves grow apart; its largest difference is reported beside,
                   and is no part of the condition.)  A measurement whose agreement fails is not timed.
  mean_steps, converged_share   from the call's outputs
  idle_share       the share of lane-iterations in which a lane of the kernel idles because its problem has stopped and
                   another of its wave of 64 has not: sum over waves of (64 * most - sum of evaluations) over
                   sum of 64 * most, with evaluations = steps + 1

Timing: wall clock around the enqueue and a synchronise of the stream (drained before, too), `steps` repetitions after
`warmup`, the two variants interleaved, per draw; median and min / max: the min - max range of one variant is the
run-to-run spread a difference has to exceed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_kinematics import FIXED, PRISMATIC, REVOLUTE, make_tree  # noqa: E402

TIPS = {"arm": 7, "body": 13}
DAMPING, MAX_STEP, TOLERANCE = 0.01, 0.5, 1e-6
CONVERGED, ITERATION_LIMIT, DEGENERATE, NOT_COMPUTABLE = 0, 1, 2, 3


def _stats(ms):
    ms = np.asarray(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4),
            "max_ms": round(float(ms.max()), 4), "steps": int(ms.size)}


def moving_links(tree, tip):
    """The chain's links that are not fixed, from the tip to the base."""
    parent, kinds = tree[0], tree[1]
    out = []
    i = tip
    while i >= 0:
        if kinds[i] != FIXED:
            out.append(i)
        i = int(parent[i])
    return out


def torch_route(torch, fk, tree, tip, targets, seeds, per_target, max_iterations):
    """The loop a caller could write: fk(q) -> poses [B, L, 16] column-major; -> (joints, status, iterations)."""
    _, kinds, index, axis, _, _ = tree
    moving = moving_links(tree, tip)
    device = seeds.device
    axes = [torch.from_numpy(np.ascontiguousarray(axis[i])).to(device) for i in moving]
    aim = targets.repeat_interleave(per_target, dim=0).view(-1, 4, 4)        # [B, column, row]
    aim_r, aim_t = aim[:, :3, :3], aim[:, 3, :3]
    q = seeds.clone()
    b = q.shape[0]
    status = torch.full((b,), -1, dtype=torch.int64, device=device)
    iterations = torch.zeros(b, dtype=torch.int32, device=device)
    damp = torch.eye(6, dtype=torch.float64, device=device) * (DAMPING * DAMPING)
    step = 0
    while True:
        poses = fk(q).view(b, -1, 4, 4)
        m = poses[:, tip]
        p = m[:, 3, :3]
        e = torch.cat([aim_t - p, torch.linalg.cross(m[:, :3, :3], aim_r, dim=2).sum(dim=1) * 0.5], dim=1)
        trace = (m[:, :3, :3] * aim_r).sum(dim=(1, 2))
        bad = ~torch.isfinite(e).all(dim=1)
        converged = (e.abs() <= TOLERANCE).all(dim=1) & (trace > 1.0)
        live = status < 0
        stop = torch.where(bad, NOT_COMPUTABLE, torch.where(converged, CONVERGED,
                                                             ITERATION_LIMIT if step >= max_iterations else -1))
        status = torch.where(live, stop, status)
        live = status < 0
        if not bool(live.any()):
            return q, status.to(torch.uint8), iterations
        columns = []
        for i, a_joint in zip(moving, axes):
            a = torch.matmul(poses[:, i, :3, :3].transpose(1, 2), a_joint)
            if kinds[i] == REVOLUTE:
                columns.append(torch.cat([torch.linalg.cross(a, p - poses[:, i, 3, :3], dim=1), a], dim=1))
            else:
                columns.append(torch.cat([a, torch.zeros_like(a)], dim=1))
        jac = torch.stack(columns, dim=2)                                     # [B, 6, M]
        y = torch.linalg.solve(torch.matmul(jac, jac.transpose(1, 2)) + damp, e.nan_to_num())
        dq = torch.matmul(jac.transpose(1, 2), y[:, :, None])[:, :, 0]
        largest = dq.abs().amax(dim=1, keepdim=True)
        dq = torch.where(largest > MAX_STEP, dq * (MAX_STEP / largest), dq)
        dq = torch.where(live[:, None], dq, torch.zeros_like(dq))
        for k, i in enumerate(moving):
            q[:, index[i]] += dq[:, k]
        iterations += live.to(torch.int32)
        step += 1


def idle_share(iterations):
    evaluations = np.asarray(iterations, dtype=np.int64) + 1
    pad = (-len(evaluations)) % 64
    waves = np.concatenate([evaluations, np.zeros(pad, np.int64)]).reshape(-1, 64)
    slots = 64 * waves.max(axis=1).sum()
    return float((slots - waves.sum()) / slots)


def problems(torch, ctx, handle, tree, tip, b, per_target, spread, seed):
    """(targets [T, 16], seeds [B, J]) on the device"""
    links, joints = len(tree[0]), tree[5]
    generator = torch.Generator(device="cuda")
    generator.manual_seed(seed)
    num_targets = b // per_target
    truth = (torch.rand((num_targets, joints), dtype=torch.float64, device="cuda", generator=generator) * 2 - 1) * 2.5
    for column in sorted({int(c) for kind, c in zip(tree[1], tree[2]) if kind == PRISMATIC}):
        truth[:, column] *= 0.1 / 2.5
    poses = torch.empty((num_targets, links, 16), dtype=torch.float64, device="cuda")
    ctx.forward_kinematics_dev(handle, truth.data_ptr(), num_targets, poses.data_ptr())
    ctx.synchronize()
    targets = poses[:, tip].contiguous()
    noise = torch.rand((num_targets * per_target, joints), dtype=torch.float64, device="cuda", generator=generator)
    seeds = truth.repeat_interleave(per_target, dim=0) + (noise * 2 - 1) * spread
    return targets, seeds.contiguous()


def one_measurement(ctx, torch, handle, tree, name, b, spread, max_iterations, draw, args):
    tip, links, joints = TIPS[name], len(tree[0]), tree[5]
    per_target = args.seeds_per_target
    targets, seeds = problems(torch, ctx, handle, tree, tip, b, per_target, spread, 1000 * draw + b % 97)
    b = seeds.shape[0]
    out = {"joints": torch.empty((b, joints), dtype=torch.float64, device="cuda"),
           "status": torch.empty(b, dtype=torch.uint8, device="cuda"),
           "iterations": torch.empty(b, dtype=torch.int32, device="cuda"),
           "error": torch.empty((b, 6), dtype=torch.float64, device="cuda"),
           "tip_pose": torch.empty((b, 16), dtype=torch.float64, device="cuda"),
           "fk_status": torch.empty(b, dtype=torch.uint8, device="cuda")}
    poses = torch.empty((b, links, 16), dtype=torch.float64, device="cuda")

    def ik():
        ctx.solve_ik_dev(handle, tip, targets.data_ptr(), targets.shape[0], seeds.data_ptr(), out["status"].data_ptr(),
                         joints_out_ptr=out["joints"].data_ptr(), iterations_ptr=out["iterations"].data_ptr(),
                         error_ptr=out["error"].data_ptr(), tip_pose_ptr=out["tip_pose"].data_ptr(),
                         fk_status_ptr=out["fk_status"].data_ptr(), seeds_per_target=per_target,
                         max_iterations=max_iterations, damping=DAMPING, max_step=MAX_STEP,
                         position_tolerance=TOLERANCE, rotation_tolerance=TOLERANCE)

    def fk(q):
        ctx.forward_kinematics_dev(handle, q.data_ptr(), b, poses.data_ptr())
        return poses

    keep = {}

    def route():
        keep["out"] = torch_route(torch, fk, tree, tip, targets, seeds, per_target, max_iterations)

    ik()
    route()
    ctx.synchronize()
    joints_route, status_route, _ = keep["out"]
    status = out["status"]
    done = (status == CONVERGED) & (status_route == CONVERGED)
    difference = (out["joints"] - joints_route).abs().amax(dim=1)
    record = {"bench": "ik", "tree": name, "links": links, "joints": joints, "chain_joints": len(moving_links(tree, tip)),
              "problems": b, "seeds_per_target": per_target, "spread": spread, "max_iterations": max_iterations,
              "draw": draw, "status_mismatches": int((status != status_route).sum().item()),
              "max_joint_difference_converged": float(difference[done].max().item()) if bool(done.any()) else 0.0,
              "max_joint_difference_other": float(difference[~done].max().item()) if bool((~done).any()) else 0.0}
    iterations = out["iterations"].cpu().numpy()
    record["statuses_converged_limit_degenerate_notcomputable"] = np.bincount(status.cpu().numpy(), minlength=4).tolist()
    record["converged_share"] = round(float((status == CONVERGED).double().mean().item()), 4)
    record["mean_steps"] = round(float(iterations.mean()), 3)
    record["idle_share"] = round(idle_share(iterations), 4)
    record["agree"] = record["status_mismatches"] == 0 and record["max_joint_difference_converged"] <= 1e-9
    if record["agree"]:
        ik_ms, route_ms = [], []
        for step in range(args.warmup + args.steps):
            for call, ms in ((ik, ik_ms), (route, route_ms)):
                ctx.synchronize()
                t0 = time.perf_counter()
                call()
                ctx.synchronize()
                if step >= args.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
        record["ik"], record["torch"] = _stats(ik_ms), _stats(route_ms)
        record["problems_per_s"] = round(b / (record["ik"]["median_ms"] * 1e-3), 1)
        record["torch_over_ik"] = round(record["torch"]["median_ms"] / record["ik"]["median_ms"], 2)
    print(json.dumps(record), flush=True)
    return record


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--problems", type=int, nargs="+", default=[10_000, 100_000, 1_000_000])
    parser.add_argument("--spreads", type=float, nargs="+", default=[0.1, 1.0])
    parser.add_argument("--iterations", type=int, nargs="+", default=[20, 100])
    parser.add_argument("--seeds-per-target", type=int, default=4)
    parser.add_argument("--trees", nargs="+", default=["arm", "body"], choices=["arm", "body"])
    parser.add_argument("--steps", type=int, default=5)
    parser.add_argument("--warmup", type=int, default=2)
    parser.add_argument("--draws", type=int, default=2)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "ik", "bench_ik.json"))
    args = parser.parse_args()

    import torch
    from voxelized_geometry_tools_amd import capi
    if not torch.cuda.is_available():
        sys.exit("bench_ik.py needs a HIP device (no CPU fallback)")
    ctx = capi.Context(0)
    ctx.set_stream(None)   # the stream torch works on
    results = []
    for name in args.trees:
        tree = make_tree(name)
        handle = ctx.kinematics(tree[0], tree[1], tree[2], tree[3], tree[4], num_joints=tree[5])
        for b in args.problems:
            for spread in args.spreads:
                for max_iterations in args.iterations:
                    for draw in range(args.draws):
                        results.append(one_measurement(ctx, torch, handle, tree, name, b, spread, max_iterations, draw, args))
                        torch.cuda.empty_cache()
        handle.close()
    ctx.reset_stream()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    if not all(r["agree"] for r in results):
        sys.exit("the torch route and the call disagree on some measurements (not timed): see `agree`")


if __name__ == "__main__":
    main()
