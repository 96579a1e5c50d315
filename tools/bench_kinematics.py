#!/usr/bin/env python3
"""Forward kinematics (vgt_hip_forward_kinematics_dev) and the joint gradient (vgt_hip_clearance_joint_gradient_dev) on
device-resident joint values, beside what a caller could do before the calls existed.  One JSON line per measurement, and
--out FILE (default profiles/kinematics/bench_kinematics.json) for all of them.

  python tools/bench_kinematics.py [--size 512] [--configurations 10000 100000 1000000] [--spheres 16 64 200]
                                   [--steps 10] [--warmup 3] [--out FILE]

Two trees: `arm`, a serial arm of 8 links (seven revolute joints and a fixed tool), and `body`, 15 links (a lift, a
shoulder bar, two arms with grippers, a camera: three branch points, one mimic column, J = 10).  Joint values are uniform
in +-pi (the lift and the grippers: +-0.1), the base stands in the middle of the grid.  Per (tree, B):

  fk               vgt_hip_forward_kinematics_dev, poses and status
  torch            the same chain as a caller could write it before: per link a [B, 4, 4] joint matrix from torch.sin /
                   torch.cos and two batched torch.matmul, the poses stacked into [B, L, 4, 4] (its own arithmetic: a
                   timing, not a parity test; the tool checks that the two agree to 1e-9)
  floor_share      the time B * (8 J + 128 L) bytes take at the HBM's 8 TB/s (the project's convention), over fk

and per (tree, B, S), on the SDF of the spheres scene at size^3, 0.01 per cell:

  check            vgt_hip_check_spheres_dev on resident poses (what the parent commit offers)
  fk+check         vgt_hip_forward_kinematics_dev, then the same check, enqueued back to back
  gradient_worst   vgt_hip_clearance_joint_gradient_dev on the check's min_sphere / min_gradient
  gradient_summed  the same call on [B, S] weights (a hinge on the clearances, about a third non-zero) and the check's
                   per-sphere gradients

Timing: wall clock around the enqueue and a synchronise of the stream (drained before, too), `steps` repetitions after
`warmup`, median and min / max: the min - max range of one variant is the run-to-run spread a difference has to exceed.
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
FIXED, REVOLUTE, PRISMATIC = 0, 1, 2


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


def _origin(rng, scale):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    m = np.eye(4)
    m[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    m[:3, 3] = (rng.random(3) - 0.3) * scale
    return m


def make_tree(name):
    """(parent, joint_type, joint_index, axis [L, 3], origin [L, 4, 4], J)"""
    rng = np.random.default_rng(7)
    if name == "arm":
        parent = [-1, 0, 1, 2, 3, 4, 5, 6]
        kinds = [REVOLUTE] * 7 + [FIXED]
        index = [0, 1, 2, 3, 4, 5, 6, 0]
        joints = 7
    else:
        parent = [-1, 0, 1, 2, 3, 4, 5, 5, 5, 2, 9, 10, 11, 11, 2]
        kinds = [FIXED, PRISMATIC, FIXED, REVOLUTE, REVOLUTE, REVOLUTE, PRISMATIC, PRISMATIC, FIXED, REVOLUTE, REVOLUTE,
                 REVOLUTE, PRISMATIC, FIXED, REVOLUTE]
        index = [0, 0, 0, 1, 2, 3, 4, 4, 0, 5, 6, 7, 8, 0, 9]
        joints = 10
    axis = rng.normal(size=(len(parent), 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    origin = np.stack([_origin(rng, 0.3) for _ in parent])
    return (np.array(parent, np.int32), np.array(kinds, np.int32), np.array(index, np.int32), axis, origin, joints)


def joint_values(torch, tree, b, seed):
    generator = torch.Generator(device="cuda")
    generator.manual_seed(seed)
    q = (torch.rand((b, tree[5]), dtype=torch.float64, device="cuda", generator=generator) * 2 - 1) * np.pi
    for column in sorted({int(column) for kind, column in zip(tree[1], tree[2]) if kind == PRISMATIC}):
        q[:, column] *= 0.1 / np.pi
    return q.contiguous()


def torch_chain(torch, tree, q, base):
    """[B, L, 4, 4] world_from_link by batched matmul: what a caller could write without the call"""
    parent, kinds, index, axis, origin, _ = tree
    b = q.shape[0]
    eye = torch.eye(4, dtype=torch.float64, device="cuda")
    origins = torch.from_numpy(origin).cuda()
    base = torch.from_numpy(base).cuda()
    poses = []
    for i in range(len(parent)):
        above = poses[parent[i]] if parent[i] >= 0 else base
        frame = torch.matmul(above, origins[i])
        if kinds[i] == FIXED:
            poses.append(frame.expand(b, 4, 4) if frame.dim() == 2 else frame)
            continue
        v = q[:, index[i]]
        joint = eye.repeat(b, 1, 1)
        a = torch.from_numpy(axis[i]).cuda()
        if kinds[i] == REVOLUTE:
            s, c = torch.sin(v)[:, None, None], torch.cos(v)[:, None, None]
            cross = torch.tensor([[0, -axis[i][2], axis[i][1]], [axis[i][2], 0, -axis[i][0]], [-axis[i][1], axis[i][0], 0]],
                                 dtype=torch.float64, device="cuda")
            joint[:, :3, :3] = c * eye[:3, :3] + (1 - c) * torch.outer(a, a) + s * cross
        else:
            joint[:, :3, 3] = v[:, None] * a
        poses.append(torch.matmul(frame, joint))
    return torch.stack(poses, dim=1)


def make_model(torch, num_spheres, num_links, seed):
    rng = np.random.default_rng(seed)
    xyzr = np.empty((num_spheres, 4))
    xyzr[:, :3] = (rng.random((num_spheres, 3)) - 0.5) * 0.2
    xyzr[:, 3] = rng.random(num_spheres) * 0.03
    link = rng.integers(0, num_links, num_spheres).astype(np.int32)
    return torch.from_numpy(xyzr).cuda(), torch.from_numpy(link).cuda()


def scene_sdf(ctx, torch, capi, synthetic, size):
    shape = (size,) * 3
    occ = torch.from_numpy(synthetic.make_occupancy(shape, "spheres", seed=42)).cuda()
    sdf = torch.empty(shape, dtype=torch.float32, device="cuda")
    nbytes = capi.sdf_workspace_bytes(shape)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ctx.sdf_dev(occ.data_ptr(), shape, RESOLUTION, sdf.data_ptr(), workspace.data_ptr(), nbytes)
    ctx.synchronize()
    return sdf


def one_tree_and_batch(ctx, torch, sdf, size, name, b, args):
    tree = make_tree(name)
    links, joints = len(tree[0]), tree[5]
    handle = ctx.kinematics(tree[0], tree[1], tree[2], tree[3], tree[4], num_joints=joints)
    base = np.eye(4)
    base[:3, 3] = size * RESOLUTION * 0.5
    q = joint_values(torch, tree, b, 100 + b % 97)
    poses = torch.empty((b, links, 16), dtype=torch.float64, device="cuda")
    fk_status = torch.empty(b, dtype=torch.uint8, device="cuda")

    def fk():
        ctx.forward_kinematics_dev(handle, q.data_ptr(), b, poses.data_ptr(), fk_status.data_ptr(), world_from_base=base)

    fk_ms = _timed(ctx, fk, args.warmup, args.steps)
    keep = {}

    def yardstick():
        keep["poses"] = torch_chain(torch, tree, q, base)

    torch_ms = _timed(ctx, yardstick, args.warmup, args.steps)
    ours = poses.view(b, links, 4, 4).transpose(2, 3)
    difference = float((ours - keep["poses"]).abs().max().item())
    del keep, ours
    record = {"bench": "kinematics", "what": "fk", "tree": name, "links": links, "joints": joints, "configurations": b,
              "fk": _stats(fk_ms), "torch": _stats(torch_ms), "max_abs_difference": difference,
              "not_computable": int((fk_status & 1).sum().item())}
    record["torch_over_fk"] = round(record["torch"]["median_ms"] / record["fk"]["median_ms"], 2)
    record["floor_bytes"] = b * (8 * joints + 128 * links)
    record["floor_share"] = round(record["floor_bytes"] / HBM_BYTES_PER_S / (record["fk"]["median_ms"] * 1e-3), 4)
    print(json.dumps(record), flush=True)
    results = [record]
    if difference > 1e-9:
        sys.exit("the torch chain and the call disagree: %g" % difference)

    shape = (size,) * 3
    for s in args.spheres:
        xyzr, link = make_model(torch, s, links, 1000 + s)
        out = {"status": torch.empty(b, dtype=torch.uint8, device="cuda"),
               "min_clearance": torch.empty(b, dtype=torch.float64, device="cuda"),
               "min_sphere": torch.empty(b, dtype=torch.int32, device="cuda"),
               "num_below": torch.empty(b, dtype=torch.int32, device="cuda"),
               "num_outside": torch.empty(b, dtype=torch.int32, device="cuda"),
               "min_gradient": torch.empty((b, 3), dtype=torch.float64, device="cuda")}
        per_sphere = {"sphere_clearance": torch.empty((b, s), dtype=torch.float64, device="cuda"),
                      "sphere_gradient": torch.empty((b, s, 3), dtype=torch.float64, device="cuda")}

        def check(extra={}):
            ctx.check_spheres_dev(sdf.data_ptr(), shape, RESOLUTION, xyzr.data_ptr(), link.data_ptr(), s,
                                  poses.data_ptr(), links, b, out["status"].data_ptr(),
                                  **{n + "_ptr": t.data_ptr() for n, t in out.items() if n != "status"},
                                  **{n + "_ptr": t.data_ptr() for n, t in extra.items()},
                                  minimum_clearance=MINIMUM_CLEARANCE)

        def both():
            fk()
            check()

        check_ms = _timed(ctx, check, args.warmup, args.steps)
        both_ms = _timed(ctx, both, args.warmup, args.steps)
        check(per_sphere)
        ctx.synchronize()
        statuses = np.bincount(out["status"].cpu().numpy(), minlength=3).tolist()
        weight = torch.clamp(0.3 - per_sphere["sphere_clearance"], min=0.0)
        weight = torch.nan_to_num(weight, nan=0.0).contiguous()
        gradient = torch.empty((b, joints), dtype=torch.float64, device="cuda")

        def worst():
            ctx.clearance_joint_gradient_dev(handle, poses.data_ptr(), b, xyzr.data_ptr(), link.data_ptr(), s,
                                             gradient.data_ptr(), min_sphere_ptr=out["min_sphere"].data_ptr(),
                                             min_gradient_ptr=out["min_gradient"].data_ptr())

        def summed():
            ctx.clearance_joint_gradient_dev(handle, poses.data_ptr(), b, xyzr.data_ptr(), link.data_ptr(), s,
                                             gradient.data_ptr(), sphere_weight_ptr=weight.data_ptr(),
                                             sphere_gradient_ptr=per_sphere["sphere_gradient"].data_ptr())

        worst_ms = _timed(ctx, worst, args.warmup, args.steps)
        summed_ms = _timed(ctx, summed, args.warmup, args.steps)
        record = {"bench": "kinematics", "what": "check", "tree": name, "links": links, "joints": joints, "size": size,
                  "configurations": b, "spheres": s, "statuses_clear_collision_novalue": statuses,
                  "weights_nonzero_share": round(float((weight != 0).double().mean().item()), 3),
                  "check": _stats(check_ms), "fk_and_check": _stats(both_ms), "gradient_worst": _stats(worst_ms),
                  "gradient_summed": _stats(summed_ms)}
        record["fk_and_check_over_check"] = round(record["fk_and_check"]["median_ms"] / record["check"]["median_ms"], 3)
        record["fk_share_of_check"] = round(results[0]["fk"]["median_ms"] / record["check"]["median_ms"], 4)
        print(json.dumps(record), flush=True)
        results.append(record)
        del per_sphere, weight, gradient, out
        torch.cuda.empty_cache()
    handle.close()
    return results


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--size", type=int, default=512)
    parser.add_argument("--configurations", type=int, nargs="+", default=[10_000, 100_000, 1_000_000])
    parser.add_argument("--spheres", type=int, nargs="+", default=[16, 64, 200])
    parser.add_argument("--trees", nargs="+", default=["arm", "body"], choices=["arm", "body"])
    parser.add_argument("--steps", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "kinematics", "bench_kinematics.json"))
    args = parser.parse_args()

    import torch
    from voxelized_geometry_tools_amd import capi, synthetic
    if not torch.cuda.is_available():
        sys.exit("bench_kinematics.py needs a HIP device (no CPU fallback)")
    ctx = capi.Context(0)
    ctx.set_stream(None)   # the stream torch works on
    sdf = scene_sdf(ctx, torch, capi, synthetic, args.size)
    results = []
    for name in args.trees:
        for b in args.configurations:
            results.extend(one_tree_and_batch(ctx, torch, sdf, args.size, name, b, args))
            torch.cuda.empty_cache()
    ctx.reset_stream()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
