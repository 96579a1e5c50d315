#!/usr/bin/env python3
"""The self-collision check (vgt_hip_check_self_collision_dev) on device-resident joint values, beside the only route a
caller had before the call existed.  One JSON line per measurement, and --out FILE (default
profiles/self/bench_self.json) for all of them.

  python tools/bench_self.py [--batches 10000 100000 1000000] [--spheres 16 64 200] [--trees arm body]
                             [--steps 10] [--warmup 3] [--out FILE] [--call-only]

The trees, the joint values and the models are those of tools/bench_kinematics.py (`arm`: 8 links, J = 7; `body`: 15
links, J = 10); no field is involved.  The pair list is vgt_hip_self_collision_pairs with the adjacency flag: every pair
of spheres on different links that are not parent and child.  Per (tree, B, S) and minimum_clearance (0, and the median
pair clearance, so that half the pairs count as below):

  call        vgt_hip_check_self_collision_dev, every per-configuration output (no pair_clearance)
  call_verdict   the same with status, num_below and min_clearance alone (no phase D)
  composed    vgt_hip_forward_kinematics_dev, then torch: the sphere links' poses gathered, the centres transformed,
              the pairs' centres by index_select, the explicit (e0 e0 + e1 e1) + e2 e2, sqrt, the two subtractions, min /
              argmin and the counts -- in chunks of configurations whose workspace stays under 4 GB (chunk and
              workspace_bytes, the peak of the allocator over the route, are recorded).  No direction, no gradient: the
              route computes less than the call.

Before anything is timed both routes are compared: status, num_below, min_pair and the bits of min_clearance.  Where
torch's bits differ the first three are still asserted and the largest difference is recorded.  A difference in those
three ends the run.

--call-only (tools/ab_self.py: builds of the kernel with other knobs): the comparison still runs, the composed route is
not timed.

Timing: wall clock around the enqueue and a synchronise of the stream (drained before, too), `steps` repetitions after
`warmup`, median and min / max: the min - max range of one variant is the run-to-run spread a difference has to exceed.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_kinematics as K  # noqa: E402

WORKSPACE_LIMIT = 4.0e9


class Composed:
    """The route before the call: forward kinematics into memory, then torch over the pairs, chunk by chunk."""

    def __init__(self, ctx, torch, handle, links, base, xyzr, link, pairs, q):
        self.ctx, self.torch, self.handle, self.links, self.base = ctx, torch, handle, links, base
        self.xyzr, self.q = xyzr, q
        self.link = link.long()
        self.a, self.b = pairs[:, 0].long().contiguous(), pairs[:, 1].long().contiguous()
        self.num, self.s, self.p = q.shape[0], xyzr.shape[0], pairs.shape[0]
        self.radii = (xyzr[:, 3][self.a], xyzr[:, 3][self.b])
        # per configuration: gathered poses S * 128, centres and their temporaries S * 24 * 3, per pair two gathered
        # centres, e, three products, d2, dist, the clearances and two masks: about 24 * 3 + 8 * 8 + 2
        per_configuration = self.s * 200 + self.p * 140 + links * 128
        self.chunk = int(max(1, min(self.num, (WORKSPACE_LIMIT * 0.8) // per_configuration)))
        self.poses = torch.empty((self.num, links, 16), dtype=torch.float64, device="cuda")
        self.fk_status = torch.empty(self.num, dtype=torch.uint8, device="cuda")
        self.status = torch.empty(self.num, dtype=torch.uint8, device="cuda")
        self.num_below = torch.empty(self.num, dtype=torch.int32, device="cuda")
        self.min_clearance = torch.empty(self.num, dtype=torch.float64, device="cuda")
        self.min_pair = torch.empty(self.num, dtype=torch.int32, device="cuda")

    def __call__(self, minimum):
        torch = self.torch
        self.ctx.forward_kinematics_dev(self.handle, self.q.data_ptr(), self.num, self.poses.data_ptr(),
                                        self.fk_status.data_ptr(), world_from_base=self.base)
        x, y, z = self.xyzr[:, 0], self.xyzr[:, 1], self.xyzr[:, 2]
        inf = torch.tensor(float("inf"), dtype=torch.float64, device="cuda")
        for first in range(0, self.num, self.chunk):
            rows = slice(first, min(self.num, first + self.chunk))
            m = self.poses[rows].index_select(1, self.link)                          # [chunk, S, 16]
            centres = torch.stack([((m[:, :, r] * x + m[:, :, 4 + r] * y) + m[:, :, 8 + r] * z) + m[:, :, 12 + r]
                                   for r in range(3)], dim=2)                        # [chunk, S, 3]
            del m
            e = centres.index_select(1, self.a) - centres.index_select(1, self.b)    # [chunk, P, 3]
            d2 = (e[:, :, 0] * e[:, :, 0] + e[:, :, 1] * e[:, :, 1]) + e[:, :, 2] * e[:, :, 2]
            del e
            clearance = (torch.sqrt(d2) - self.radii[0]) - self.radii[1]
            del d2
            value = ~torch.isnan(clearance)
            below = (value & (clearance <= minimum)).sum(dim=1, dtype=torch.int32)
            least, where = torch.where(value, clearance, inf).min(dim=1)
            found = value.any(dim=1)
            self.num_below[rows] = below
            self.min_clearance[rows] = torch.where(found, least, torch.full_like(least, float("nan")))
            self.min_pair[rows] = torch.where(found, where, torch.full_like(where, -1)).int()
            self.status[rows] = torch.where(below > 0, 1, torch.where(found, 0, 2)).to(torch.uint8)


def one_tree_and_batch(ctx, torch, capi, name, b, args):
    tree = K.make_tree(name)
    links, joints = len(tree[0]), tree[5]
    handle = ctx.kinematics(tree[0], tree[1], tree[2], tree[3], tree[4], num_joints=joints)
    base = np.eye(4)
    q = K.joint_values(torch, tree, b, 300 + b % 97)
    results = []
    for s in args.spheres:
        xyzr, link = K.make_model(torch, s, links, 1000 + s)
        listed, count = capi.self_collision_pairs(link.cpu().numpy(), links, parent=tree[0], skip_adjacent=True)
        assert count == len(listed) and count > 0
        pairs = torch.from_numpy(listed).cuda()
        p = len(listed)
        out = {"status": torch.empty(b, dtype=torch.uint8, device="cuda"),
               "num_below": torch.empty(b, dtype=torch.int32, device="cuda"),
               "num_without_value": torch.empty(b, dtype=torch.int32, device="cuda"),
               "min_clearance": torch.empty(b, dtype=torch.float64, device="cuda"),
               "min_pair": torch.empty(b, dtype=torch.int32, device="cuda"),
               "min_direction": torch.empty((b, 3), dtype=torch.float64, device="cuda"),
               "joint_gradient": torch.empty((b, joints), dtype=torch.float64, device="cuda"),
               "fk_status": torch.empty(b, dtype=torch.uint8, device="cuda")}
        verdict = ("num_below", "min_clearance")

        def fused(minimum, everything=True):
            ctx.check_self_collision_dev(xyzr.data_ptr(), link.data_ptr(), s, pairs.data_ptr(), p, handle, q.data_ptr(),
                                         b, out["status"].data_ptr(), minimum_clearance=minimum, world_from_base=base,
                                         **{k + "_ptr": t.data_ptr() for k, t in out.items()
                                            if k != "status" and (everything or k in verdict)})

        route = Composed(ctx, torch, handle, links, base, xyzr, link, pairs, q)
        fused(0.0)
        ctx.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        route(0.0)
        ctx.synchronize()
        workspace = int(torch.cuda.max_memory_allocated() - before) + route.poses.numel() * 8
        # the median pair clearance, from a sample of configurations
        sample = Composed(ctx, torch, handle, links, base, xyzr, link, pairs, q[:min(b, 256)].contiguous())
        sample.chunk = min(b, 256)
        sample(0.0)
        m = sample.poses.index_select(1, sample.link)
        x, y, z = xyzr[:, 0], xyzr[:, 1], xyzr[:, 2]
        centres = torch.stack([((m[:, :, r] * x + m[:, :, 4 + r] * y) + m[:, :, 8 + r] * z) + m[:, :, 12 + r]
                               for r in range(3)], dim=2)
        e = centres.index_select(1, sample.a) - centres.index_select(1, sample.b)
        all_clearances = (torch.sqrt((e[:, :, 0] * e[:, :, 0] + e[:, :, 1] * e[:, :, 1]) + e[:, :, 2] * e[:, :, 2])
                          - sample.radii[0]) - sample.radii[1]
        median = float(all_clearances[torch.isfinite(all_clearances)].median().item())
        del sample, m, centres, e, all_clearances
        for minimum in (0.0, median):
            # ---- both routes agree, before anything is timed ----
            route(minimum)
            fused(minimum)
            ctx.synchronize()
            agree = {"status": bool((out["status"] == route.status).all().item()),
                     "num_below": bool((out["num_below"] == route.num_below).all().item()),
                     "min_pair": bool((out["min_pair"] == route.min_pair).all().item())}
            same = out["min_clearance"].view(torch.int64) == route.min_clearance.view(torch.int64)
            both_nan = torch.isnan(out["min_clearance"]) & torch.isnan(route.min_clearance)
            agree["min_clearance_bits"] = bool((same | both_nan).all().item())
            difference = float(torch.nan_to_num(out["min_clearance"] - route.min_clearance).abs().max().item())
            if not (agree["status"] and agree["num_below"] and agree["min_pair"]):
                sys.exit("the composed route and the call disagree: %s" % json.dumps(agree))
            below_share = float(out["num_below"].double().sum().item()) / max(1, b * p)
            collisions = float((out["status"] == 1).double().mean().item())
            kept = out["min_clearance"].clone()
            fused(minimum, False)
            ctx.synchronize()
            if not bool((out["min_clearance"].view(torch.int64) == kept.view(torch.int64)).all().item()):
                sys.exit("the verdict-only call and the call disagree")
            del kept, same, both_nan
            # ---- timings ----
            call_ms = K._timed(ctx, lambda: fused(minimum), args.warmup, args.steps)
            verdict_ms = K._timed(ctx, lambda: fused(minimum, False), args.warmup, args.steps)
            record = {"bench": "self", "tree": name, "links": links, "joints": joints, "configurations": b, "spheres": s,
                      "pairs": p, "minimum_clearance": round(minimum, 6), "below_share": round(below_share, 4),
                      "collision_share": round(collisions, 4),
                      "tile_samples": capi.self_collision_tile_samples(links, s), "agree": agree,
                      "largest_min_clearance_difference": difference, "call_ms": K._stats(call_ms),
                      "call_verdict_ms": K._stats(verdict_ms)}
            record["pair_tests_per_ns"] = round(b * p / (record["call_ms"]["median_ms"] * 1e6), 3)
            if not args.call_only:
                route_ms = K._timed(ctx, lambda: route(minimum), args.warmup, args.steps)
                record.update(composed_ms=K._stats(route_ms), chunk=route.chunk, workspace_bytes=workspace)
                record["composed_over_call"] = round(record["composed_ms"]["median_ms"] / record["call_ms"]["median_ms"], 3)
            print(json.dumps(record), flush=True)
            results.append(record)
        del route, out
        torch.cuda.empty_cache()
    handle.close()
    return results


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--batches", type=int, nargs="+", default=[10000, 100000, 1000000])
    parser.add_argument("--spheres", type=int, nargs="+", default=[16, 64, 200])
    parser.add_argument("--trees", nargs="+", default=["arm", "body"], choices=["arm", "body"])
    parser.add_argument("--steps", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "self", "bench_self.json"))
    parser.add_argument("--call-only", action="store_true")
    args = parser.parse_args()

    import torch
    from voxelized_geometry_tools_amd import capi
    if not torch.cuda.is_available():
        sys.exit("bench_self.py needs a HIP device (no CPU fallback)")
    ctx = capi.Context(0)
    ctx.set_stream(None)   # the stream torch works on
    results = []
    for name in args.trees:
        for b in args.batches:
            results.extend(one_tree_and_batch(ctx, torch, capi, name, b, args))
            torch.cuda.empty_cache()
    ctx.reset_stream()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(row) for row in results) + "\n]\n")   # (one row per line)


if __name__ == "__main__":
    main()
