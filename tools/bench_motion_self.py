#!/usr/bin/env python3
"""Motion checks with the self part (vgt_hip_check_motions_with_self_dev) on device-resident endpoints, beside the only
route a caller had before the call existed.  One JSON line per measurement, and --out FILE (default
profiles/motion_self/bench_motion_self.json) for all of them.

  python tools/bench_motion_self.py [--size 512] [--shapes 10000x31 10000x99 100000x9] [--spheres 16 64 200]
                                    [--trees arm body] [--steps 10] [--warmup 3] [--out FILE] [--call-only]

The trees, the joint values, the models, the field and the endpoints are those of tools/bench_motions.py; the pair list is
vgt_hip_self_collision_pairs with the adjacency flag, as in tools/bench_self.py.  A shape ExN is E motions of N steps
(N + 1 samples each).  Per (tree, shape, S), without and with stop_at_collision:

  call       vgt_hip_check_motions_with_self_dev, all eleven outputs
  composed   a torch interpolation to [E (N + 1), J] with the two endpoints' own bits; vgt_hip_check_motions_dev on the
             endpoints (its seven outputs); vgt_hip_check_self_collision_dev on the flat samples (status, min_clearance,
             min_pair, fk_status), in chunks of motions whose samples stay under 4 GB; and a torch reduction per motion:
             the first self collision, the least self clearance, the combined status and first collision.  The route
             cannot stop across the two checks: with the flag it runs as without it.

Thresholds: without the flag the kinematics bench's 0.02 for the field and 0 for the pairs; with it the medians of the
motions' min_clearance and self_min_clearance, so that at least half the motions collide (the same for both routes).

Before anything is timed both routes are compared, without the flag: status, first_collision and the bits of
min_clearance and self_min_clearance; with the flag status and first_collision, which it does not change.  A difference
ends the run.

--call-only (an A/B of builds of the kernel with other knobs, VGT_HIP_LIB naming the library): the comparison still runs,
the composed route is not timed.

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
import bench_motions as M  # noqa: E402

WORKSPACE_LIMIT = 4.0e9


class Composed:
    """The route before the call: interpolate, the two checks that exist, reduce per motion."""

    def __init__(self, ctx, torch, sdf, shape, handle, joints, base, xyzr, link, pairs, joint_from, joint_to, n):
        self.ctx, self.torch, self.sdf, self.shape, self.handle, self.base = ctx, torch, sdf, shape, handle, base
        self.xyzr, self.link, self.pairs, self.a, self.b, self.n = xyzr, link, pairs, joint_from, joint_to, n
        self.e = e = joint_from.shape[0]
        count = e * (n + 1)
        # per motion: its samples' joint values and their temporaries, the four per-sample outputs
        per_motion = (n + 1) * (max(joints, 1) * 8 * 3 + 14)
        self.chunk = int(max(1, min(e, (WORKSPACE_LIMIT * 0.8) // per_motion)))
        # (tensor by tensor: a division by a Python number is a multiplication by its reciprocal, which is not k / n)
        steps = torch.full((n + 1,), float(max(n, 1)), dtype=torch.float64, device="cuda")
        self.t = (torch.arange(n + 1, dtype=torch.float64, device="cuda") / steps)[None, :, None]
        self.self_status = torch.empty(count, dtype=torch.uint8, device="cuda")
        self.self_clearance = torch.empty(count, dtype=torch.float64, device="cuda")
        self.self_pair = torch.empty(count, dtype=torch.int32, device="cuda")
        self.self_fk = torch.empty(count, dtype=torch.uint8, device="cuda")
        self.motion = {"status": torch.empty(e, dtype=torch.uint8, device="cuda"),
                       "first_collision": torch.empty(e, dtype=torch.int32, device="cuda"),
                       "min_clearance": torch.empty(e, dtype=torch.float64, device="cuda"),
                       "min_sample": torch.empty(e, dtype=torch.int32, device="cuda"),
                       "min_sphere": torch.empty(e, dtype=torch.int32, device="cuda"),
                       "min_gradient": torch.empty((e, 3), dtype=torch.float64, device="cuda"),
                       "fk_status": torch.empty(e, dtype=torch.uint8, device="cuda")}
        self.result = None

    def __call__(self, minimum_clearance, self_minimum_clearance):
        torch, e, n, s = self.torch, self.e, self.n, self.xyzr.shape[0]
        self.ctx.check_motions_dev(self.sdf.data_ptr(), self.shape, K.RESOLUTION, self.xyzr.data_ptr(),
                                   self.link.data_ptr(), s, self.handle, self.a.data_ptr(), self.b.data_ptr(), n, e,
                                   self.motion["status"].data_ptr(),
                                   **{k + "_ptr": t.data_ptr() for k, t in self.motion.items() if k != "status"},
                                   minimum_clearance=minimum_clearance, world_from_base=self.base)
        for first in range(0, e, self.chunk):
            rows = slice(first, min(e, first + self.chunk))
            a, b = self.a[rows], self.b[rows]
            q = a[:, None, :] + self.t * (b - a)[:, None, :]
            q[:, 0] = a                                                  # (the endpoints' own bits, as the call takes them)
            if n > 0:
                q[:, n] = b
            num = q.shape[0] * (n + 1)
            q = q.reshape(num, -1).contiguous()
            at = first * (n + 1)
            self.ctx.check_self_collision_dev(self.xyzr.data_ptr(), self.link.data_ptr(), s, self.pairs.data_ptr(),
                                              self.pairs.shape[0], self.handle, q.data_ptr(), num,
                                              self.self_status[at:].data_ptr(),
                                              minimum_clearance=self_minimum_clearance,
                                              min_clearance_ptr=self.self_clearance[at:].data_ptr(),
                                              min_pair_ptr=self.self_pair[at:].data_ptr(),
                                              fk_status_ptr=self.self_fk[at:].data_ptr(), world_from_base=self.base)
            del q
        status = self.self_status.view(e, n + 1)
        collides = status == 1
        any_self = collides.any(dim=1)
        first_self = torch.where(any_self, collides.to(torch.int8).argmax(dim=1), torch.full_like(any_self, n + 1, dtype=torch.int64))
        theirs = self.motion["first_collision"].long()
        first_field = torch.where(theirs >= 0, theirs, torch.full_like(theirs, n + 1))
        first = torch.minimum(first_self, first_field)
        collision = first <= n
        cause = ((first_field == first) & collision).to(torch.uint8) | (((first_self == first) & collision).to(torch.uint8) << 1)
        no_value = (self.motion["status"] == 2) | (status == 2).any(dim=1)
        verdict = torch.where(collision, 1, torch.where(no_value, 2, 0)).to(torch.uint8)
        clearance = torch.nan_to_num(self.self_clearance, nan=float("inf")).view(e, n + 1)
        least, sample = clearance.min(dim=1)
        found = torch.isfinite(least) | (least < 0)
        rows = torch.arange(e, device="cuda") * (n + 1) + sample
        pair = self.self_pair[rows]
        self.result = {"status": verdict, "first_collision": torch.where(collision, first, torch.full_like(first, -1)).int(),
                       "collision_cause": cause, "min_clearance": self.motion["min_clearance"],
                       "self_min_clearance": torch.where(found, least, torch.full_like(least, float("nan"))),
                       "self_min_sample": sample, "self_min_pair": pair}


def same_bits(torch, a, b):
    return bool(((a.view(torch.int64) == b.view(torch.int64)) | (torch.isnan(a) & torch.isnan(b))).all().item())


def one_tree_and_shape(ctx, torch, capi, sdf, size, name, motions, n, args):
    tree = K.make_tree(name)
    links, joints = len(tree[0]), tree[5]
    handle = ctx.kinematics(tree[0], tree[1], tree[2], tree[3], tree[4], num_joints=joints)
    base = np.eye(4)
    base[:3, 3] = size * K.RESOLUTION * 0.5
    joint_from, joint_to = M.endpoints(torch, tree, motions, 200 + motions % 97)
    shape = (size,) * 3
    results = []
    for s in args.spheres:
        xyzr, link = K.make_model(torch, s, links, 1000 + s)
        listed, count = capi.self_collision_pairs(link.cpu().numpy(), links, parent=tree[0], skip_adjacent=True)
        assert count == len(listed) and count > 0
        pairs = torch.from_numpy(listed).cuda()
        p = len(listed)
        kinds = {"status": torch.uint8, "first_collision": torch.int32, "collision_cause": torch.uint8,
                 "min_clearance": torch.float64, "min_sample": torch.int32, "min_sphere": torch.int32,
                 "min_gradient": torch.float64, "self_min_clearance": torch.float64, "self_min_sample": torch.int32,
                 "self_min_pair": torch.int32, "fk_status": torch.uint8}
        out = {k: torch.empty((motions, 3) if k == "min_gradient" else motions, dtype=d, device="cuda")
               for k, d in kinds.items()}

        def fused(minimum, self_minimum, stop):
            ctx.check_motions_with_self_dev(sdf.data_ptr(), shape, K.RESOLUTION, xyzr.data_ptr(), link.data_ptr(), s,
                                            pairs.data_ptr(), p, handle, joint_from.data_ptr(), joint_to.data_ptr(), n,
                                            motions, out["status"].data_ptr(),
                                            **{k + "_ptr": t.data_ptr() for k, t in out.items() if k != "status"},
                                            minimum_clearance=minimum, self_minimum_clearance=self_minimum,
                                            stop_at_collision=stop, world_from_base=base)

        route = Composed(ctx, torch, sdf, shape, handle, joints, base, xyzr, link, pairs, joint_from, joint_to, n)
        fused(K.MINIMUM_CLEARANCE, 0.0, False)
        ctx.synchronize()
        finite = out["min_clearance"][torch.isfinite(out["min_clearance"])]
        half = float(finite.median().item()) if finite.numel() else K.MINIMUM_CLEARANCE
        finite = out["self_min_clearance"][torch.isfinite(out["self_min_clearance"])]
        self_half = float(finite.median().item()) if finite.numel() else 0.0
        for stop, minimum, self_minimum in ((False, K.MINIMUM_CLEARANCE, 0.0), (True, half, self_half)):
            # ---- both routes agree, before anything is timed ----
            route(minimum, self_minimum)
            fused(minimum, self_minimum, False)
            ctx.synchronize()
            agree = {k: bool((out[k] == route.result[k]).all().item()) for k in ("status", "first_collision", "collision_cause")}
            agree["min_clearance_bits"] = same_bits(torch, out["min_clearance"], route.result["min_clearance"])
            agree["self_min_clearance_bits"] = same_bits(torch, out["self_min_clearance"], route.result["self_min_clearance"])
            if stop:
                fused(minimum, self_minimum, True)
                ctx.synchronize()
                agree["status_with_stop"] = bool((out["status"] == route.result["status"]).all().item())
                agree["first_collision_with_stop"] = bool((out["first_collision"] == route.result["first_collision"]).all().item())
            if not all(agree.values()):
                apart = torch.nan_to_num(out["self_min_clearance"] - route.result["self_min_clearance"]).abs()
                sys.exit("the composed route and the call disagree: %s (self_min_clearance: %d motions apart, at most %g)"
                         % (json.dumps(agree), int((apart > 0).sum().item()), float(apart.max().item())))
            statuses = np.bincount(out["status"].cpu().numpy(), minlength=4).tolist()
            causes = np.bincount(out["collision_cause"].cpu().numpy(), minlength=4).tolist()
            # ---- timings ----
            call_ms = K._timed(ctx, lambda: fused(minimum, self_minimum, stop), args.warmup, args.steps)
            record = {"bench": "motion_self", "tree": name, "links": links, "joints": joints, "size": size,
                      "motions": motions, "steps_per_motion": n, "spheres": s, "pairs": p, "stop_at_collision": stop,
                      "minimum_clearance": round(minimum, 6), "self_minimum_clearance": round(self_minimum, 6),
                      "tile_samples": capi.motion_self_tile_samples(links, s),
                      "statuses_clear_collision_novalue_invalid": statuses, "causes_none_field_self_both": causes,
                      "agree": agree, "call_ms": K._stats(call_ms)}
            record["samples_per_us"] = round(motions * (n + 1) / (record["call_ms"]["median_ms"] * 1e3), 2)
            if not args.call_only:
                route_ms = K._timed(ctx, lambda: route(minimum, self_minimum), args.warmup, args.steps)
                record.update(composed_ms=K._stats(route_ms), chunk_motions=route.chunk)
                record["composed_over_call"] = round(record["composed_ms"]["median_ms"] / record["call_ms"]["median_ms"], 3)
            print(json.dumps(record), flush=True)
            results.append(record)
        del route, out
        torch.cuda.empty_cache()
    handle.close()
    return results


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--size", type=int, default=512)
    parser.add_argument("--shapes", nargs="+", default=["10000x31", "10000x99", "100000x9"])
    parser.add_argument("--spheres", type=int, nargs="+", default=[16, 64, 200])
    parser.add_argument("--trees", nargs="+", default=["arm", "body"], choices=["arm", "body"])
    parser.add_argument("--steps", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_self", "bench_motion_self.json"))
    parser.add_argument("--call-only", action="store_true")
    args = parser.parse_args()

    import torch
    from voxelized_geometry_tools_amd import capi, synthetic
    if not torch.cuda.is_available():
        sys.exit("bench_motion_self.py needs a HIP device (no CPU fallback)")
    ctx = capi.Context(0)
    ctx.set_stream(None)   # the stream torch works on
    sdf = K.scene_sdf(ctx, torch, capi, synthetic, args.size)
    results = []
    for name in args.trees:
        for shape in args.shapes:
            motions, n = (int(v) for v in shape.split("x"))
            results.extend(one_tree_and_shape(ctx, torch, capi, sdf, args.size, name, motions, n, args))
            torch.cuda.empty_cache()
    ctx.reset_stream()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(row) for row in results) + "\n]\n")   # (one row per line)


if __name__ == "__main__":
    main()
