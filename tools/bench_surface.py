#!/usr/bin/env python3
"""Time of the surface extraction (vgt_hip_extract_surface*) on signed distance fields of the benchmark's occupancy
grids, beside a pass of the same class (vgt_hip_select_cells_dev, SELECT_SURFACE_26, on the occupancy) and, at 256^3,
the vectorised numpy restatement of tests/surface_ref.py.  One JSON line per case.

  python tools/bench_surface.py [--sizes 256 512 1024] [--dists spheres salt] [--steps 20] [--warmup 3]
                                [--host-steps 3] [--numpy-max 256] [--out profiles/surface/bench_surface.json]

Timing: wall clock around the call (every call ends with the read-back of the counts and a drained stream; a
vgt_hip_synchronize before and after brackets it), `steps` repetitions after `warmup`, median and min / max.
  count        extract_surface_dev without outputs: mark, face mark, two scans, the counts to the host
  extract      the same with output buffers of exactly the counts (vertices, vertex cells, triangles stay on the device):
               what a caller pays who knows the counts or over-allocates
  host         vgt_hip_extract_surface twice (count, then fetch), field and mesh in host memory, as
               Context.extract_surface does it; `host-steps` repetitions
Floor convention: the extraction must read the field once (4 B/voxel) and write the mesh (24 B + 4 B per vertex, 12 B per
triangle) at the HBM peak of 8000 GB/s; the bit planes, the second read of the 8 corners of active cubes and the
neighbour columns of the mark are what the design adds.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBPS = 8000.0


def _stats(ms, prefix=""):
    ms = np.asarray(ms)
    return {prefix + "median_ms": round(float(np.median(ms)), 4), prefix + "min_ms": round(float(ms.min()), 4),
            prefix + "max_ms": round(float(ms.max()), 4), prefix + "steps": int(ms.size)}


def _timed(ctx, call, warmup, steps):
    ms, result = [], None
    for step in range(warmup + steps):
        ctx.synchronize()
        t0 = time.perf_counter()
        result = call()
        ctx.synchronize()
        if step >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms, result


def main():
    import ctypes
    import torch
    from voxelized_geometry_tools_amd import capi, synthetic

    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--dists", nargs="+", default=["spheres", "salt"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--numpy-max", type=int, default=256)
    ap.add_argument("--resolution", type=float, default=0.02)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(record):
        line = json.dumps(record)
        print(line, flush=True)
        lines.append(line)

    ctx = capi.Context(0)
    for size in args.sizes:
        shape = (size, size, size)
        vox = size ** 3
        for dist in args.dists:
            print("# %s %d^3: occupancy and its signed distance field" % (dist, size), flush=True)
            occ_dev = torch.from_numpy(synthetic.make_occupancy(shape, dist, seed=42)).cuda()
            sdf_dev = torch.empty(shape, dtype=torch.float32, device="cuda")
            ws_bytes = capi.sdf_workspace_bytes(shape)
            ws_dev = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.sdf_dev(occ_dev.data_ptr(), shape, args.resolution, sdf_dev.data_ptr(), ws_dev.data_ptr(), ws_bytes)
            ctx.synchronize()
            del ws_dev
            nv, nt = ctypes.c_int64(0), ctypes.c_int64(0)

            def run(vertices=None, cells=None, triangles=None):
                capi.check(ctx._lib.vgt_hip_extract_surface_dev(
                    ctx.handle, sdf_dev.data_ptr(), *shape, 0.0, 0, args.resolution, None,
                    None if vertices is None else vertices.data_ptr(), None if cells is None else cells.data_ptr(),
                    0 if vertices is None else len(vertices), None if triangles is None else triangles.data_ptr(),
                    0 if triangles is None else len(triangles), ctypes.byref(nv), ctypes.byref(nt)))
                return int(nv.value), int(nt.value)

            num_vertices, num_triangles = run()
            vertices = torch.empty((max(num_vertices, 1), 3), dtype=torch.float64, device="cuda")
            cells = torch.empty(max(num_vertices, 1), dtype=torch.int32, device="cuda")
            triangles = torch.empty((max(num_triangles, 1), 3), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            count_ms, _ = _timed(ctx, run, args.warmup, args.steps)
            ms, got = _timed(ctx, lambda: run(vertices, cells, triangles), args.warmup, args.steps)
            assert got == (num_vertices, num_triangles)
            rec = {"case": "extract_surface_dev", "dist": dist, "shape": list(shape), "resolution": args.resolution,
                   "vertices": num_vertices, "triangles": num_triangles}
            rec.update(_stats(ms))
            rec["count_only_median_ms"] = _stats(count_ms)["median_ms"]
            output_bytes = 28 * num_vertices + 12 * num_triangles
            floor_bytes = 4 * vox + output_bytes
            med = rec["median_ms"] * 1e-3
            rec["output_bytes"] = output_bytes
            rec["floor_bytes"] = floor_bytes
            rec["floor"] = "4 B/voxel read + the mesh written at %g GB/s" % HBM_PEAK_GBPS
            rec["fraction_of_hbm_floor"] = round(floor_bytes / med / 1e9 / HBM_PEAK_GBPS, 4)
            rec["voxels_per_s"] = round(vox / med, 1)
            # the pass of the same class: the 26-neighbour surface cells of the occupancy
            selected = ctx.select_cells_dev(occ_dev.data_ptr(), shape, capi.SELECT_SURFACE_26, 15)
            indices = torch.empty(max(selected, 1), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            select_ms, _ = _timed(ctx, lambda: ctx.select_cells_dev(occ_dev.data_ptr(), shape, capi.SELECT_SURFACE_26, 15,
                                                                    0.5, None, indices.data_ptr(), None, None, selected),
                                  args.warmup, args.steps)
            rec["select_surface_26_cells"] = selected
            rec["select_surface_26_median_ms"] = _stats(select_ms)["median_ms"]
            rec["extract_over_select_surface_26"] = round(rec["median_ms"] / rec["select_surface_26_median_ms"], 2)
            del indices, occ_dev
            # host to host
            sdf_host = sdf_dev.cpu().numpy()
            host_ms, mesh = _timed(ctx, lambda: ctx.extract_surface(sdf_host, args.resolution, with_cells=True), 1,
                                   args.host_steps)
            rec.update(_stats(host_ms, "host_"))
            rec["host_equals_device"] = bool(
                np.array_equal(mesh[0].view(np.uint64), vertices[:num_vertices].cpu().numpy().view(np.uint64)) and
                np.array_equal(mesh[1], triangles[:num_triangles].cpu().numpy()) and
                np.array_equal(mesh[2], cells[:num_vertices].cpu().numpy()))
            if size <= args.numpy_max:
                import surface_ref
                t0 = time.perf_counter()
                want = surface_ref.extract(sdf_host, args.resolution)
                rec["numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                rec["numpy_equals_device"] = bool(all(a.tobytes() == b.tobytes() for a, b in zip(want, mesh)))
                rec["numpy_over_host"] = round(rec["numpy_ms"] / rec["host_median_ms"], 1)
            emit(rec)
            del vertices, cells, triangles, sdf_dev, sdf_host, mesh
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
