#!/usr/bin/env python3
"""Times the mesh rasterizer and mesh -> SDF on one device, device-resident, and writes profiles/mesh/bench_mesh.json.

Per configuration (icosphere and triangle soup, two resolutions each): the time of one vgt_hip_rasterize_mesh_dev call
(set-up kernels, the read-back of its findings, the brick kernel; host clock around a call that ends in a stream
synchronise), the same with the map replaced by one far away from the mesh (no candidate cells: the set-up alone), the
difference as the brick kernel's time with candidate cells per second, and the time of Context.mesh_sdf's device part
(rasterize + sdf_dev).  Warm-up calls first, then `--repeats` timed calls; median, minimum and maximum are reported.
Kernel times proper come from a rocprofv3 --kernel-trace --stats run of this script (profiles/mesh/)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from voxelized_geometry_tools_amd import capi, synthetic  # noqa: E402


def candidate_cells(vertices, triangles, origin, shape, resolution):
    """Cells of the triangles' index ranges (clamped to the grid), as the set-up kernel counts them."""
    p = vertices[triangles]                                   # [T, 3, 3]
    inv = 1.0 / resolution
    lo = np.floor((p.min(axis=1) - origin) * inv).astype(np.int64)
    hi = np.floor((p.max(axis=1) - origin) * inv).astype(np.int64)
    lo = np.maximum(lo, 0)
    hi = np.minimum(hi, np.asarray(shape) - 1)
    return int(np.prod(np.maximum(hi - lo + 1, 0), axis=1).sum())


def spread(samples_ms):
    return {"median_ms": statistics.median(samples_ms), "min_ms": min(samples_ms), "max_ms": max(samples_ms),
            "repeats": len(samples_ms)}


def timed(fn, sync, warmup, repeats):
    for _ in range(warmup):
        fn()
    sync()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--only", default=None, help="run one configuration (by name), e.g. under a profiler")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh", "bench_mesh.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh.py needs a HIP device (no CPU fallback)")
    configs = []
    for res in (0.01, 0.005):
        v, t = synthetic.mesh_icosphere(5, 1.27, (0.013, -0.007, 0.021))
        configs.append(("icosphere_20480_res%g" % res, v, t, res))
    for res in (0.02, 0.01):
        v, t = synthetic.mesh_triangle_soup(100_000, (0.0, 0.0, 0.0), (4.0, 4.0, 4.0), 0.08, seed=42)
        configs.append(("soup_100000_res%g" % res, v, t, res))
    results = {"device": capi.device_name(0), "warmup": args.warmup, "configs": {}}
    with capi.Context(0) as ctx:
        for name, v, t, res in configs:
            if args.only and name != args.only:
                continue
            shape, origin = capi.mesh_grid_for(v, res)
            wfg = synthetic.translation_xform(*origin)
            gfw = synthetic.translation_xform(*(-origin))
            far = synthetic.translation_xform(*(origin + 1.0e4)), synthetic.translation_xform(*(-(origin + 1.0e4)))
            v_dev = torch.from_numpy(np.ascontiguousarray(v)).cuda()
            t_dev = torch.from_numpy(np.ascontiguousarray(t)).cuda()
            occ_dev = torch.zeros(shape, dtype=torch.float32, device="cuda")
            sdf_dev = torch.empty(shape, dtype=torch.float32, device="cuda")
            ws_bytes = capi.sdf_workspace_bytes(shape)
            ws_dev = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
            minmax_dev = torch.empty(2, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            entry = {"triangles": int(len(t)), "grid": list(shape), "resolution": res,
                     "candidate_cells": candidate_cells(v, t, origin, shape, res)}
            for rule in (0, 1):
                def rasterize(xf=(wfg, gfw), rule=rule):
                    ctx.rasterize_mesh_dev(v_dev.data_ptr(), len(v), t_dev.data_ptr(), len(t), occ_dev.data_ptr(), 4,
                                           shape, res, xf[0], xf[1], False, rule)

                def chain(rule=rule):
                    occ_dev.zero_()
                    torch.cuda.synchronize()
                    rasterize()
                    ctx.sdf_dev(occ_dev.data_ptr(), shape, res, sdf_dev.data_ptr(), ws_dev.data_ptr(), ws_bytes,
                                minmax_dev.data_ptr())

                call = timed(rasterize, ctx.synchronize, args.warmup, args.repeats)
                setup = timed(lambda: rasterize(far), ctx.synchronize, args.warmup, args.repeats)
                sdf = timed(chain, ctx.synchronize, args.warmup, args.repeats)
                bricks_ms = statistics.median(call) - statistics.median(setup)
                entry["rule%d" % rule] = {
                    "rasterize_call": spread(call), "setup_only_call": spread(setup),
                    "brick_kernel_ms_by_difference": bricks_ms,
                    "candidate_cells_per_s_brick_kernel": entry["candidate_cells"] / (bricks_ms * 1e-3) if bricks_ms > 0 else None,
                    "candidate_cells_per_s_whole_call": entry["candidate_cells"] / (statistics.median(call) * 1e-3),
                    "triangles_per_s_setup": len(t) / (statistics.median(setup) * 1e-3),
                    "mesh_sdf_zero_rasterize_sdf": spread(sdf)}
            results["configs"][name] = entry
            print(json.dumps({name: entry}), flush=True)
            del occ_dev, sdf_dev, ws_dev
    if not args.only:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
