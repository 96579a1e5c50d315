#!/usr/bin/env python3
"""Device-resident time of the cell selection (vgt_hip_select_cells_dev) beside the only route to the same list that
existed before it: vgt_hip_component_surface_mask_dev, the mask to the host, numpy.flatnonzero.  One JSON line per case.

  python tools/bench_select.py [--sizes 256 512 1024] [--dists spheres salt] [--steps 20] [--warmup 3]
                               [--mask-steps 5] [--out FILE]

Timing: wall clock around the call (it ends with the read-back of the count and a drained stream; a
vgt_hip_synchronize before and after brackets it), `steps` repetitions after `warmup`, median and min / max.
  compact        select_cells_dev with output buffers of exactly the count: mark, scan, count to the host, emit; the
                 lists stay on the device
  compact+d2h    the same, then the int32 indices to the host: the point at which the mask route has its list
  mask route     (VGT_HIP_SELECT_COMPONENT_SURFACE only: the 26-neighbour rule had no device form) the dense mask, its
                 copy to the host, flatnonzero; `mask-steps` repetitions, it takes seconds at 1024^3
Floor convention: the selection must read the values (4 B/voxel) and, for the component rule, the labels (4 B/voxel more)
at the HBM peak of 8000 GB/s; the bit grid (1/8 B/voxel written, then read) and the lists are what the design adds.
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
    import torch
    from voxelized_geometry_tools_amd import capi, synthetic

    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--dists", nargs="+", default=["spheres", "salt"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mask-steps", type=int, default=5)
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
            occ_dev = torch.from_numpy(synthetic.make_occupancy(shape, dist, seed=42)).cuda()
            labels_dev = torch.empty(shape, dtype=torch.int32, device="cuda")
            components = ctx.connected_components_dev(occ_dev.data_ptr(), shape, labels_dev.data_ptr())
            for rule, name, class_mask, floor_bytes in (
                    (capi.SELECT_SURFACE_26, "surface_26", 15, 4),
                    (capi.SELECT_COMPONENT_SURFACE, "component_surface", capi.CLASS_ABOVE, 8)):
                needs_labels = rule == capi.SELECT_COMPONENT_SURFACE
                lab_ptr = labels_dev.data_ptr() if needs_labels else None
                count = ctx.select_cells_dev(occ_dev.data_ptr(), shape, rule, class_mask, 0.5, lab_ptr)
                indices_dev = torch.empty(max(count, 1), dtype=torch.int32, device="cuda")
                payload_dev = torch.empty(max(count, 1), dtype=torch.int32, device="cuda") if needs_labels else None
                pay_ptr = payload_dev.data_ptr() if needs_labels else None

                def compact():
                    return ctx.select_cells_dev(occ_dev.data_ptr(), shape, rule, class_mask, 0.5, lab_ptr,
                                                indices_dev.data_ptr(), None, pay_ptr, count)

                def compact_to_host():
                    compact()
                    return indices_dev[:count].cpu().numpy()

                count_ms, _ = _timed(ctx, lambda: ctx.select_cells_dev(occ_dev.data_ptr(), shape, rule, class_mask, 0.5,
                                                                       lab_ptr), args.warmup, args.steps)
                ms, got = _timed(ctx, compact, args.warmup, args.steps)
                host_ms, host_list = _timed(ctx, compact_to_host, args.warmup, args.steps)
                rec = {"case": "select_cells_dev", "rule": name, "class_mask": class_mask, "dist": dist,
                       "shape": list(shape), "components": components, "selected": count,
                       "selected_fraction": round(count / vox, 6)}
                rec.update(_stats(ms))
                med = rec["median_ms"] * 1e-3
                rec["count_only_median_ms"] = _stats(count_ms)["median_ms"]
                rec["to_host_median_ms"] = _stats(host_ms)["median_ms"]
                rec["voxels_per_s"] = round(vox / med, 1)
                rec["floor"] = "%d B/voxel read at %g GB/s" % (floor_bytes, HBM_PEAK_GBPS)
                rec["fraction_of_hbm_floor"] = round(floor_bytes * vox / med / 1e9 / HBM_PEAK_GBPS, 4)
                if needs_labels:
                    mask_dev = torch.empty(shape, dtype=torch.uint8, device="cuda")

                    def mask_route():
                        ctx.component_surface_mask_dev(occ_dev.data_ptr(), labels_dev.data_ptr(), shape, class_mask,
                                                       mask_dev.data_ptr())
                        ctx.synchronize()
                        return np.flatnonzero(mask_dev.cpu().numpy().reshape(-1))

                    def mask_kernel():
                        ctx.component_surface_mask_dev(occ_dev.data_ptr(), labels_dev.data_ptr(), shape, class_mask,
                                                       mask_dev.data_ptr())

                    kernel_ms, _ = _timed(ctx, mask_kernel, args.warmup, args.steps)
                    route_ms, want = _timed(ctx, mask_route, 1, args.mask_steps)
                    rec.update(_stats(route_ms, "mask_route_"))
                    rec["mask_kernel_median_ms"] = _stats(kernel_ms)["median_ms"]
                    rec["equal_to_mask_route"] = bool(got == count and np.array_equal(host_list, want))
                    rec["mask_route_over_compact_to_host"] = round(rec["mask_route_median_ms"] /
                                                                   rec["to_host_median_ms"], 2)
                    del mask_dev
                emit(rec)
                del indices_dev, payload_dev
            del occ_dev, labels_dev
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
