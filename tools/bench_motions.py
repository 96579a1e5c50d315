#!/usr/bin/env python3
"""Motion checks (vgt_hip_check_motions_dev) on device-resident endpoints, beside the only route a caller had before the
call existed.  One JSON line per measurement, and --out FILE (default profiles/motions/bench_motions.json) for all of
them.

  python tools/bench_motions.py [--size 512] [--shapes 10000x31 10000x99 100000x9] [--spheres 16 64 200]
                                [--trees arm body] [--steps 10] [--warmup 3] [--out FILE]

The trees, the joint values, the models and the field are those of tools/bench_kinematics.py (`arm`: 8 links, J = 7;
`body`: 15 links, J = 10; the SDF of the spheres scene at size^3, 0.01 per cell; the base in the middle of the grid).
A shape ExN is E motions of N steps (N + 1 samples each); joint_to = joint_from + uniform in +-0.5 (the lift and the
grippers: +-0.02).  Per (tree, shape, S), without and with stop_at_collision:

  motions      vgt_hip_check_motions_dev, all seven outputs
  three_calls  a torch interpolation to [E (N + 1), J], vgt_hip_forward_kinematics_dev, vgt_hip_check_spheres_dev, and a
               torch reshape / min / argmax per motion (entry points this call does not touch; its last sample is
               a + 1 (b - a), so its answers may differ from the call's in the last bits: a timing, and the tool records
               the share of motions whose status agrees)
  pose_workspace_bytes   what that route holds in between: E (N + 1) L 128 bytes

minimum_clearance: without the flag the kinematics bench's 0.02; with it the median of the motions' min_clearance, so that
about half the motions collide (the same threshold for both routes; the three calls cannot stop early).

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


def endpoints(torch, tree, motions, seed):
    joint_from = K.joint_values(torch, tree, motions, seed)
    generator = torch.Generator(device="cuda")
    generator.manual_seed(seed + 1)
    step = (torch.rand(joint_from.shape, dtype=torch.float64, device="cuda", generator=generator) * 2 - 1) * 0.5
    for column in sorted({int(column) for kind, column in zip(tree[1], tree[2]) if kind == K.PRISMATIC}):
        step[:, column] *= 0.04
    return joint_from, (joint_from + step).contiguous()


class ThreeCalls:
    """The route before the call: interpolate, forward kinematics, check, reduce per motion."""

    def __init__(self, ctx, torch, sdf, shape, handle, links, base, xyzr, link, joint_from, joint_to, n):
        self.ctx, self.torch, self.sdf, self.shape, self.handle, self.links, self.base = ctx, torch, sdf, shape, handle, links, base
        self.xyzr, self.link, self.a, self.b, self.n = xyzr, link, joint_from, joint_to, n
        self.e = joint_from.shape[0]
        count = self.e * (n + 1)
        self.poses = torch.empty((count, links, 16), dtype=torch.float64, device="cuda")
        self.fk_status = torch.empty(count, dtype=torch.uint8, device="cuda")
        self.out = {"status": torch.empty(count, dtype=torch.uint8, device="cuda"),
                    "min_clearance": torch.empty(count, dtype=torch.float64, device="cuda"),
                    "min_sphere": torch.empty(count, dtype=torch.int32, device="cuda"),
                    "min_gradient": torch.empty((count, 3), dtype=torch.float64, device="cuda")}
        self.t = (torch.arange(n + 1, dtype=torch.float64, device="cuda") / max(n, 1))[None, :, None]
        self.result = None

    def pose_bytes(self):
        return self.poses.numel() * 8

    def __call__(self, minimum_clearance):
        torch, e, n = self.torch, self.e, self.n
        q = (self.a[:, None, :] + self.t * (self.b - self.a)[:, None, :]).reshape(e * (n + 1), -1).contiguous()
        self.ctx.forward_kinematics_dev(self.handle, q.data_ptr(), e * (n + 1), self.poses.data_ptr(),
                                        self.fk_status.data_ptr(), world_from_base=self.base)
        self.ctx.check_spheres_dev(self.sdf.data_ptr(), self.shape, K.RESOLUTION, self.xyzr.data_ptr(),
                                   self.link.data_ptr(), self.xyzr.shape[0], self.poses.data_ptr(), self.links,
                                   e * (n + 1), self.out["status"].data_ptr(),
                                   min_clearance_ptr=self.out["min_clearance"].data_ptr(),
                                   min_sphere_ptr=self.out["min_sphere"].data_ptr(),
                                   min_gradient_ptr=self.out["min_gradient"].data_ptr(),
                                   minimum_clearance=minimum_clearance)
        status = self.out["status"].view(e, n + 1)
        collides = status == 1
        any_collision = collides.any(dim=1)
        first = torch.where(any_collision, collides.to(torch.int8).argmax(dim=1), torch.full_like(any_collision, -1, dtype=torch.int64))
        no_value = (status == 2).any(dim=1)
        verdict = torch.where(any_collision, 1, torch.where(no_value, 2, 0)).to(torch.uint8)
        clearance = torch.nan_to_num(self.out["min_clearance"], nan=float("inf")).view(e, n + 1)
        least, sample = clearance.min(dim=1)
        rows = torch.arange(e, device="cuda") * (n + 1) + sample
        sphere = self.out["min_sphere"][rows]
        gradient = self.out["min_gradient"][rows]
        fk = self.fk_status.view(e, n + 1)
        fk_bits = (fk & 1).amax(dim=1) | (fk & 2).amax(dim=1)
        self.result = (verdict, first, least, sample, sphere, gradient, fk_bits)


def one_tree_and_shape(ctx, torch, sdf, size, name, motions, n, args):
    tree = K.make_tree(name)
    links, joints = len(tree[0]), tree[5]
    handle = ctx.kinematics(tree[0], tree[1], tree[2], tree[3], tree[4], num_joints=joints)
    base = np.eye(4)
    base[:3, 3] = size * K.RESOLUTION * 0.5
    joint_from, joint_to = endpoints(torch, tree, motions, 200 + motions % 97)
    shape = (size,) * 3
    results = []
    for s in args.spheres:
        xyzr, link = K.make_model(torch, s, links, 1000 + s)
        out = {"status": torch.empty(motions, dtype=torch.uint8, device="cuda"),
               "first_collision": torch.empty(motions, dtype=torch.int32, device="cuda"),
               "min_clearance": torch.empty(motions, dtype=torch.float64, device="cuda"),
               "min_sample": torch.empty(motions, dtype=torch.int32, device="cuda"),
               "min_sphere": torch.empty(motions, dtype=torch.int32, device="cuda"),
               "min_gradient": torch.empty((motions, 3), dtype=torch.float64, device="cuda"),
               "fk_status": torch.empty(motions, dtype=torch.uint8, device="cuda")}

        def fused(minimum_clearance, stop):
            ctx.check_motions_dev(sdf.data_ptr(), shape, K.RESOLUTION, xyzr.data_ptr(), link.data_ptr(), s, handle,
                                  joint_from.data_ptr(), joint_to.data_ptr(), n, motions, out["status"].data_ptr(),
                                  **{k + "_ptr": t.data_ptr() for k, t in out.items() if k != "status"},
                                  minimum_clearance=minimum_clearance, stop_at_collision=stop, world_from_base=base)

        route = ThreeCalls(ctx, torch, sdf, shape, handle, links, base, xyzr, link, joint_from, joint_to, n)
        fused(K.MINIMUM_CLEARANCE, False)
        ctx.synchronize()
        finite = out["min_clearance"][torch.isfinite(out["min_clearance"])]
        half = float(finite.median().item()) if finite.numel() else K.MINIMUM_CLEARANCE
        for stop, threshold in ((False, K.MINIMUM_CLEARANCE), (True, half)):
            fused_ms = K._timed(ctx, lambda: fused(threshold, stop), args.warmup, args.steps)
            route_ms = K._timed(ctx, lambda: route(threshold), args.warmup, args.steps)
            fused(threshold, False)   # (the route cannot stop: the comparison of the answers is without the flag)
            ctx.synchronize()
            statuses = np.bincount(out["status"].cpu().numpy(), minlength=4).tolist()
            agree = float((out["status"] == route.result[0]).double().mean().item())
            record = {"bench": "motions", "tree": name, "links": links, "joints": joints, "size": size, "motions": motions,
                      "steps_per_motion": n, "spheres": s, "stop_at_collision": stop, "minimum_clearance": round(threshold, 6),
                      "tile_samples": capi_tile(links), "statuses_clear_collision_novalue_invalid": statuses,
                      "status_agreement": round(agree, 5), "motions_ms": K._stats(fused_ms),
                      "three_calls_ms": K._stats(route_ms), "pose_workspace_bytes": route.pose_bytes()}
            record["three_calls_over_motions"] = round(record["three_calls_ms"]["median_ms"] / record["motions_ms"]["median_ms"], 3)
            record["samples_per_us"] = round(motions * (n + 1) / (record["motions_ms"]["median_ms"] * 1e3), 2)
            print(json.dumps(record), flush=True)
            results.append(record)
            if agree < 0.99:
                sys.exit("the three calls and the call disagree on %.3f of the motions" % (1.0 - agree))
        del route, out
        torch.cuda.empty_cache()
    handle.close()
    return results


def capi_tile(links):
    from voxelized_geometry_tools_amd import capi
    return capi.motion_tile_samples(links)


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--size", type=int, default=512)
    parser.add_argument("--shapes", nargs="+", default=["10000x31", "10000x99", "100000x9"])
    parser.add_argument("--spheres", type=int, nargs="+", default=[16, 64, 200])
    parser.add_argument("--trees", nargs="+", default=["arm", "body"], choices=["arm", "body"])
    parser.add_argument("--steps", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "motions", "bench_motions.json"))
    args = parser.parse_args()

    import torch
    from voxelized_geometry_tools_amd import capi, synthetic
    if not torch.cuda.is_available():
        sys.exit("bench_motions.py needs a HIP device (no CPU fallback)")
    ctx = capi.Context(0)
    ctx.set_stream(None)   # the stream torch works on
    sdf = K.scene_sdf(ctx, torch, capi, synthetic, args.size)
    results = []
    for name in args.trees:
        for shape in args.shapes:
            motions, n = (int(v) for v in shape.split("x"))
            results.extend(one_tree_and_shape(ctx, torch, sdf, args.size, name, motions, n, args))
            torch.cuda.empty_cache()
    ctx.reset_stream()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
