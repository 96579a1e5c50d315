#!/usr/bin/env python3
"""The clearance cost and its joint gradient (vgt_hip_clearance_cost_dev) on device-resident joint values, beside the only
route a caller had before the call existed.  One JSON line per measurement, and --out FILE (default
profiles/cost/bench_cost.json) for all of them.

  python tools/bench_cost.py [--size 512] [--batches 10000 100000 1000000] [--spheres 16 64 200] [--trees arm body]
                             [--steps 10] [--warmup 3] [--out FILE] [--call-only]

The trees, the joint values, the models and the field are those of tools/bench_kinematics.py (`arm`: 8 links, J = 7;
`body`: 15 links, J = 10; the SDF of the spheres scene at size^3, 0.01 per cell; the base in the middle of the grid).
Per (tree, B, S) and margin:

  cost           vgt_hip_clearance_cost_dev, all six outputs
  cost_only      the same with joint_gradient and num_without_gradient NULL (roll-out scoring)
  composed       vgt_hip_forward_kinematics_dev, vgt_hip_check_spheres_dev with both per-sphere outputs, the hinge and
                 the NaN-gradient rule in torch, the summed vgt_hip_clearance_joint_gradient_dev, a torch sum for the cost
                 (entry points this call does not touch)
  composed_cost_only   that route without its gradient step
  workspace_bytes      what the composed route holds in between: poses B L 128, clearances B S 8, gradients B S 24,
                       weights B S 8 and costs B S 8

Margins: the median of the finite clearances, so that about half the spheres are active; and 1e-6, where only the
penetrating spheres are.

Before anything is timed both routes are compared: the counts, the gradient bit for bit, and the cost bit for bit
against the sum of the route's per-sphere costs added column by column in ascending s (the order of the definition;
torch.sum, which the timed route uses, adds in an order of its own: the share of configurations where it gives the
same bits is recorded as torch_sum_same_bits).  A difference ends the run.

--call-only (tools/ab_cost.py: builds of the kernel with other knobs): the comparison still runs, the composed route is
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

FEW_ACTIVE_MARGIN = 1e-6


class Composed:
    """The route before the call: forward kinematics, check with per-sphere outputs, torch hinge, summed gradient."""

    def __init__(self, ctx, torch, sdf, shape, handle, links, joints, base, xyzr, link, q):
        self.ctx, self.torch, self.sdf, self.shape, self.handle, self.links, self.base = ctx, torch, sdf, shape, handle, links, base
        self.xyzr, self.link, self.q = xyzr, link, q
        self.b, self.s = q.shape[0], xyzr.shape[0]
        b, s = self.b, self.s
        self.poses = torch.empty((b, links, 16), dtype=torch.float64, device="cuda")
        self.fk_status = torch.empty(b, dtype=torch.uint8, device="cuda")
        self.status = torch.empty(b, dtype=torch.uint8, device="cuda")
        self.clearance = torch.empty((b, s), dtype=torch.float64, device="cuda")
        self.gradient = torch.empty((b, s, 3), dtype=torch.float64, device="cuda")
        self.joint_gradient = torch.empty((b, joints), dtype=torch.float64, device="cuda")
        self.result = None

    def workspace_bytes(self):
        return self.poses.numel() * 8 + self.clearance.numel() * 8 * 3 + self.gradient.numel() * 8

    def hinge(self, margin):
        torch, d = self.torch, self.clearance
        # (a tensor on the device, not a Python number: torch divides by a host scalar by multiplying with its reciprocal,
        # which is not the division of the definition)
        eps = torch.tensor(margin, dtype=torch.float64, device="cuda")
        value = ~torch.isnan(d)
        below = d < 0.0
        inside = value & ~below & (d <= eps)
        t = d - eps
        c = torch.where(below, (eps * 0.5) - d, torch.where(inside, ((t * t) * 0.5) / eps, torch.zeros_like(d)))
        w = torch.where(below, torch.full_like(d, -1.0), torch.where(inside, t / eps, torch.zeros_like(d)))
        c = torch.where(value, c, torch.zeros_like(d))     # (no contribution: + 0.0 leaves a sum of costs >= +0.0 as it is)
        return value, c, w

    def __call__(self, margin, with_gradient=True):
        torch, b, s = self.torch, self.b, self.s
        self.ctx.forward_kinematics_dev(self.handle, self.q.data_ptr(), b, self.poses.data_ptr(), self.fk_status.data_ptr(),
                                        world_from_base=self.base)
        self.ctx.check_spheres_dev(self.sdf.data_ptr(), self.shape, K.RESOLUTION, self.xyzr.data_ptr(), self.link.data_ptr(),
                                   s, self.poses.data_ptr(), self.links, b, self.status.data_ptr(),
                                   sphere_clearance_ptr=self.clearance.data_ptr(),
                                   sphere_gradient_ptr=self.gradient.data_ptr() if with_gradient else None)
        value, c, w = self.hinge(margin)
        active = value & (w != 0.0)
        num_active = active.sum(dim=1, dtype=torch.int32)
        num_outside = (~value).sum(dim=1, dtype=torch.int32)
        cost = c.sum(dim=1)
        if not with_gradient:
            self.result = (cost, None, num_active, num_outside, None, self.fk_status, c)
            return
        without = active & torch.isnan(self.gradient).any(dim=2)
        weight = torch.where(without, torch.zeros_like(w), w).contiguous()
        self.ctx.clearance_joint_gradient_dev(self.handle, self.poses.data_ptr(), b, self.xyzr.data_ptr(),
                                              self.link.data_ptr(), s, self.joint_gradient.data_ptr(),
                                              sphere_weight_ptr=weight.data_ptr(),
                                              sphere_gradient_ptr=self.gradient.data_ptr())
        self.result = (cost, self.joint_gradient, num_active, num_outside, without.sum(dim=1, dtype=torch.int32),
                       self.fk_status, c)


def same_bits(torch, a, b):
    if a.dtype != torch.float64:
        return bool((a == b).all().item())
    nan_a, nan_b = torch.isnan(a), torch.isnan(b)
    return bool((nan_a == nan_b).all().item()) and bool((a[~nan_a].view(torch.int64) == b[~nan_b].view(torch.int64)).all().item())


def one_tree_and_batch(ctx, torch, capi, sdf, size, name, b, args):
    tree = K.make_tree(name)
    links, joints = len(tree[0]), tree[5]
    handle = ctx.kinematics(tree[0], tree[1], tree[2], tree[3], tree[4], num_joints=joints)
    base = np.eye(4)
    base[:3, 3] = size * K.RESOLUTION * 0.5
    q = K.joint_values(torch, tree, b, 300 + b % 97)
    shape = (size,) * 3
    results = []
    for s in args.spheres:
        xyzr, link = K.make_model(torch, s, links, 1000 + s)
        out = {"cost": torch.empty(b, dtype=torch.float64, device="cuda"),
               "joint_gradient": torch.empty((b, joints), dtype=torch.float64, device="cuda"),
               "num_active": torch.empty(b, dtype=torch.int32, device="cuda"),
               "num_outside": torch.empty(b, dtype=torch.int32, device="cuda"),
               "num_without_gradient": torch.empty(b, dtype=torch.int32, device="cuda"),
               "fk_status": torch.empty(b, dtype=torch.uint8, device="cuda")}

        def fused(margin, with_gradient=True):
            skip = () if with_gradient else ("joint_gradient", "num_without_gradient")
            ctx.clearance_cost_dev(sdf.data_ptr(), shape, K.RESOLUTION, xyzr.data_ptr(), link.data_ptr(), s, handle,
                                   q.data_ptr(), b, margin, out["cost"].data_ptr(), world_from_base=base,
                                   **{k + "_ptr": t.data_ptr() for k, t in out.items() if k != "cost" and k not in skip})

        route = Composed(ctx, torch, sdf, shape, handle, links, joints, base, xyzr, link, q)
        route(1.0)
        ctx.synchronize()
        finite = route.clearance[torch.isfinite(route.clearance)]
        half = float(finite.median().item()) if finite.numel() else 0.05
        if not half > 0.0:
            half = 0.05
        for margin in (half, FEW_ACTIVE_MARGIN):
            # ---- both routes agree, before anything is timed ----
            route(margin)
            fused(margin)
            ctx.synchronize()
            cost, gradient, num_active, num_outside, num_without, fk_status, c = route.result
            ordered = torch.zeros(b, dtype=torch.float64, device="cuda")
            for column in range(s):
                ordered = ordered + c[:, column]
            agree = {"cost": same_bits(torch, out["cost"], ordered),
                     "joint_gradient": same_bits(torch, out["joint_gradient"], gradient),
                     "num_active": same_bits(torch, out["num_active"], num_active),
                     "num_outside": same_bits(torch, out["num_outside"], num_outside),
                     "num_without_gradient": same_bits(torch, out["num_without_gradient"], num_without),
                     "fk_status": same_bits(torch, out["fk_status"], fk_status)}
            torch_sum_same = float((cost.view(torch.int64) == out["cost"].view(torch.int64)).double().mean().item())
            active_share = float(out["num_active"].double().sum().item()) / max(1, b * s)
            kept = out["cost"].clone()
            fused(margin, False)
            ctx.synchronize()
            agree["cost_only"] = same_bits(torch, out["cost"], kept)
            if not all(agree.values()):
                sys.exit("the composed route and the call disagree: %s" % json.dumps(agree))
            del ordered, cost, gradient, c, kept
            route.result = None
            # ---- timings ----
            fused_ms = K._timed(ctx, lambda: fused(margin), args.warmup, args.steps)
            fused_only_ms = K._timed(ctx, lambda: fused(margin, False), args.warmup, args.steps)
            if args.call_only:
                record = {"bench": "cost", "tree": name, "links": links, "joints": joints, "size": size,
                          "configurations": b, "spheres": s, "margin": round(margin, 6),
                          "active_share": round(active_share, 4), "tile_samples": capi.cost_tile_samples(links),
                          "agree": agree, "cost_ms": K._stats(fused_ms), "cost_only_ms": K._stats(fused_only_ms)}
                print(json.dumps(record), flush=True)
                results.append(record)
                continue
            route_ms = K._timed(ctx, lambda: route(margin), args.warmup, args.steps)
            route_only_ms = K._timed(ctx, lambda: route(margin, False), args.warmup, args.steps)
            route.result = None
            record = {"bench": "cost", "tree": name, "links": links, "joints": joints, "size": size, "configurations": b,
                      "spheres": s, "margin": round(margin, 6), "active_share": round(active_share, 4),
                      "tile_samples": capi.cost_tile_samples(links), "agree": agree,
                      "torch_sum_same_bits": round(torch_sum_same, 5), "cost_ms": K._stats(fused_ms),
                      "composed_ms": K._stats(route_ms), "cost_only_ms": K._stats(fused_only_ms),
                      "composed_cost_only_ms": K._stats(route_only_ms), "workspace_bytes": route.workspace_bytes()}
            record["composed_over_cost"] = round(record["composed_ms"]["median_ms"] / record["cost_ms"]["median_ms"], 3)
            record["composed_over_cost_only"] = round(
                record["composed_cost_only_ms"]["median_ms"] / record["cost_only_ms"]["median_ms"], 3)
            record["sphere_checks_per_us"] = round(b * s / (record["cost_ms"]["median_ms"] * 1e3), 2)
            print(json.dumps(record), flush=True)
            results.append(record)
        del route, out
        torch.cuda.empty_cache()
    handle.close()
    return results


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--size", type=int, default=512)
    parser.add_argument("--batches", type=int, nargs="+", default=[10000, 100000, 1000000])
    parser.add_argument("--spheres", type=int, nargs="+", default=[16, 64, 200])
    parser.add_argument("--trees", nargs="+", default=["arm", "body"], choices=["arm", "body"])
    parser.add_argument("--steps", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "cost", "bench_cost.json"))
    parser.add_argument("--call-only", action="store_true")
    args = parser.parse_args()

    import torch
    from voxelized_geometry_tools_amd import capi, synthetic
    if not torch.cuda.is_available():
        sys.exit("bench_cost.py needs a HIP device (no CPU fallback)")
    ctx = capi.Context(0)
    ctx.set_stream(None)   # the stream torch works on
    sdf = K.scene_sdf(ctx, torch, capi, synthetic, args.size)
    results = []
    for name in args.trees:
        for b in args.batches:
            results.extend(one_tree_and_batch(ctx, torch, capi, sdf, args.size, name, b, args))
            torch.cuda.empty_cache()
    ctx.reset_stream()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
