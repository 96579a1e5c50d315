#!/usr/bin/env python3
"""Segment casts (vgt_hip_cast_segments_dev) on device-resident fields.  One JSON line per measurement, and --out FILE
(default profiles/segments/bench_segments.json) for all of them.

  python tools/bench_segments.py [--sizes 256 512] [--segments 1000000] [--steps 20] [--warmup 3] [--label TEXT]
                                 [--skip-depth-image] [--out FILE]

  (a) The spheres scene (D1) at size^3, 0.01 per cell, and its SDF extracted on the device; `segments` segments with both
      ends uniform in the grid's box; occupancy mode and SDF mode (threshold 0.02, with and without the min outputs),
      each with and without WALK_THROUGH.  Reported: ms, segments/s, cells examined/s and the bytes of field the casts
      read (4 bytes per examined cell; the load-ahead fetches up to `depth` further cells per segment, which the kernel
      throws away and which are not counted).
  (b) The yardstick: 1024 x 1024 segments that share one origin -- a depth image -- through an empty 256^3 map, beside
      vgt_hip_raycast_points_f64 on the same rays.  Both walk identical cells (the tool checks that the tracking counts
      add up to the cells examined); the raycaster also does an atomic per cell, and its entry point takes its points
      from the host (24 MB), so the casts are timed a second time with the upload of their 48 MB of segments included.

Timing: wall clock around the blocking call (the stream drained before and after), `steps` repetitions after `warmup`,
median and min / max: the min-max range of one variant is the run-to-run spread that a difference between two variants
has to exceed.  --label names the build in the records (the A/B of the load-ahead depth runs this tool once per build,
with VGT_HIP_LIB pointing at it).
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RESOLUTION = 0.01
THRESHOLD = 0.02


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


class Outputs:
    def __init__(self, torch, n):
        self.status = torch.empty(n, dtype=torch.uint8, device="cuda")
        self.hit_index = torch.empty(n, dtype=torch.int32, device="cuda")
        self.hit_fraction = torch.empty(n, dtype=torch.float64, device="cuda")
        self.cells_examined = torch.empty(n, dtype=torch.int32, device="cuda")
        self.min_value = torch.empty(n, dtype=torch.float32, device="cuda")
        self.min_index = torch.empty(n, dtype=torch.int32, device="cuda")


def _cast(ctx, field, shape, segments, n, out, mode, walk_through, with_min):
    ctx.cast_segments_dev(field.data_ptr(), shape, RESOLUTION, segments.data_ptr(), n, out.status.data_ptr(),
                          out.hit_index.data_ptr(), out.hit_fraction.data_ptr(), out.cells_examined.data_ptr(),
                          out.min_value.data_ptr() if with_min else None, out.min_index.data_ptr() if with_min else None,
                          mode=mode, unknown_is_filled=True, threshold=THRESHOLD, walk_through=walk_through)


def _record(ms, n, out):
    examined = int(out.cells_examined.sum(dtype=__import__("torch").int64).item())
    stats = _stats(ms)
    seconds = stats["median_ms"] * 1e-3
    stats.update({"segments_per_s": round(n / seconds), "cells_examined": examined,
                  "cells_examined_per_s": round(examined / seconds), "field_bytes_read": 4 * examined,
                  "statuses": np.bincount(out.status.cpu().numpy(), minlength=4).tolist()})
    return stats


def scene_casts(ctx, torch, capi, synthetic, size, n, args):
    shape = (size,) * 3
    occ = torch.from_numpy(synthetic.make_occupancy(shape, "spheres", seed=42)).cuda()
    sdf = torch.empty(shape, dtype=torch.float32, device="cuda")
    nbytes = capi.sdf_workspace_bytes(shape)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ctx.sdf_dev(occ.data_ptr(), shape, RESOLUTION, sdf.data_ptr(), workspace.data_ptr(), nbytes)
    ctx.synchronize()
    del workspace
    segments = torch.from_numpy(np.random.default_rng(7).random((n, 6)) * (size * RESOLUTION)).cuda()
    out = Outputs(torch, n)
    records = []
    variants = [("occupancy", capi.SEGMENT_OCCUPANCY, occ, False), ("sdf_below", capi.SEGMENT_SDF_BELOW, sdf, False),
                ("sdf_below+min", capi.SEGMENT_SDF_BELOW, sdf, True)]
    for name, mode, field, with_min in variants:
        for walk_through in (False, True):
            ms = _timed(ctx, lambda: _cast(ctx, field, shape, segments, n, out, mode, walk_through, with_min),
                        args.warmup, args.steps)
            record = {"bench": "segments", "label": args.label, "scene": "spheres", "size": size, "segments": n,
                      "mode": name, "walk_through": walk_through, "field_bytes": 4 * size ** 3}
            record.update(_record(ms, n, out))
            records.append(record)
            print(json.dumps(record), flush=True)
    return records


def depth_image(ctx, torch, capi, synthetic, args):
    """1024 x 1024 rays of a pinhole camera in the middle of an empty 256^3 map, each 4 m long (they all leave the map)."""
    size, side = 256, 1024
    shape = (size,) * 3
    n = side * side
    origin = np.array([1.28 + 0.003, 1.28 + 0.002, 1.28 + 0.001])
    u, v = np.meshgrid(np.linspace(-1.0, 1.0, side), np.linspace(-1.0, 1.0, side), indexing="ij")
    direction = np.stack([np.ones_like(u), u, v], axis=-1).reshape(n, 3)
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    points = direction * 4.0                                 # in the camera frame: the grid frame shifted to the origin
    segments_host = np.concatenate([np.broadcast_to(origin, (n, 3)), points + origin], axis=1)
    segments_host = np.ascontiguousarray(segments_host)
    field = torch.zeros(shape, dtype=torch.float32, device="cuda")
    segments = torch.from_numpy(segments_host).cuda()
    out = Outputs(torch, n)
    cast_ms = _timed(ctx, lambda: _cast(ctx, field, shape, segments, n, out, capi.SEGMENT_OCCUPANCY, False, False),
                     args.warmup, args.steps)
    record = {"bench": "segments_depth_image", "label": args.label, "size": size, "segments": n,
              "cast_segments_dev": _record(cast_ms, n, out)}
    pinned = torch.from_numpy(segments_host).pin_memory()

    def upload_and_cast():
        segments.copy_(pinned, non_blocking=False)
        _cast(ctx, field, shape, segments, n, out, capi.SEGMENT_OCCUPANCY, False, False)

    record["cast_segments_dev_with_upload"] = _stats(_timed(ctx, upload_and_cast, args.warmup, args.steps))
    grids = ctx.tracking_grids(size ** 3, 1)
    xform = synthetic.translation_xform(*origin)
    sizes = [size * RESOLUTION] * 3

    def raycast():
        grids.raycast_f64(0, points, 10.0, xform, RESOLUTION, 1.0 / RESOLUTION, sizes, shape)

    grids.clear()
    raycast()
    ctx.synchronize()
    visits = int(grids.retrieve(0, shape).astype(np.int64).sum())
    record["raycast_points_f64"] = _stats(_timed(ctx, raycast, args.warmup, args.steps))
    record["raycast_visits"] = visits
    record["same_cells"] = visits == record["cast_segments_dev"]["cells_examined"]
    grids.close()
    print(json.dumps(record), flush=True)
    return [record]


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    parser.add_argument("--segments", type=int, default=1_000_000)
    parser.add_argument("--steps", type=int, default=20)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--label", default="")
    parser.add_argument("--skip-depth-image", action="store_true")
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "segments", "bench_segments.json"))
    args = parser.parse_args()

    import torch
    from voxelized_geometry_tools_amd import capi, synthetic
    if not torch.cuda.is_available():
        sys.exit("bench_segments.py needs a HIP device (no CPU fallback)")
    ctx = capi.Context(0)
    ctx.set_stream(None)   # the stream torch works on
    results = []
    for size in args.sizes:
        results += scene_casts(ctx, torch, capi, synthetic, size, args.segments, args)
    if not args.skip_depth_image:
        results += depth_image(ctx, torch, capi, synthetic, args)
    ctx.reset_stream()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
