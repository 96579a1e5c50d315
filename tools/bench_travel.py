#!/usr/bin/env python3
"""Time of the cost-to-go field (vgt_hip_travel_cost_dev) on the benchmark's occupancy grids, device-resident, beside the
library's other whole-grid graph traversal (vgt_hip_connected_components_dev) on the same grid in the same run.  One
JSON line per case.

  python tools/bench_travel.py [--sizes 256 512 1024] [--dists spheres salt] [--steps 20] [--warmup 3]
                               [--heap-size 256] [--paths 1000000] [--out profiles/travel/bench_travel.json]

Cases per grid: one source (the first passable cell in linear order: the corner, or the cell nearest to it), weights
{10, 14, 17}, no limit, cost + toward + count; at the largest size also the SDF threshold form on the grid's own signed
distance field, and a cost_limit chosen (from the unlimited field's costs) to reach about a tenth of the grid.  At the
smallest size: `paths` traced paths from random reached cells (vgt_hip_trace_paths_dev, 256 cells each at most), and at
--heap-size cubed from host arrays the ratio to the heap restatement of tests/travel_ref.py (a python loop: 5 s at
48^3, a quarter of an hour at 256^3; 0 skips it).

Timing: wall clock around the call (it returns with every output complete and the stream drained; a vgt_hip_synchronize
before brackets it), `steps` repetitions after `warmup`, median and min / max.  rounds and tile runs come from the head of
the workspace (vgt_hip.h); active_share = tile runs / (rounds * tiles), the mean share of tiles that did work per round.
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
    ap.add_argument("--heap-size", type=int, default=256)
    ap.add_argument("--paths", type=int, default=1000000)
    ap.add_argument("--resolution", type=float, default=0.02)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(record):
        line = json.dumps(record)
        print(line, flush=True)
        lines.append(line)

    ctx = capi.Context(0)
    weights = (10, 14, 17)
    for size in args.sizes:
        shape = (size, size, size)
        vox = size ** 3
        tiles = ((size + 7) // 8) ** 2 * ((size + 15) // 16)
        for dist in args.dists:
            print("# %s %d^3" % (dist, size), flush=True)
            occ_host = synthetic.make_occupancy(shape, dist, seed=42)
            source = int(np.argmax(~(occ_host.reshape(-1) >= 0.5)))
            occ_dev = torch.from_numpy(occ_host).cuda()
            src_dev = torch.tensor([source], dtype=torch.int32, device="cuda")
            cost = torch.empty(shape, dtype=torch.int32, device="cuda")
            toward = torch.empty(shape, dtype=torch.int32, device="cuda")
            ws_bytes = capi.travel_cost_workspace_bytes(shape)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()

            def run(field=occ_dev, limit=capi.TRAVEL_NO_LIMIT, **kw):
                return ctx.travel_cost_dev(field.data_ptr(), shape, src_dev.data_ptr(), 1, cost.data_ptr(), ws.data_ptr(),
                                           ws_bytes, toward_ptr=toward.data_ptr(), weights=weights, cost_limit=limit, **kw)

            def record(case, ms, reached, extra=None):
                head = ws[:32].cpu().numpy()
                rounds = int(head[8:12].view(np.uint32)[0])
                tile_runs = int(head[24:32].view(np.uint64)[0])
                rec = {"case": case, "dist": dist, "shape": list(shape), "weights": list(weights), "source": source,
                       "reached": reached, "rounds": rounds, "tiles": tiles, "tile_runs": tile_runs,
                       "active_share": round(tile_runs / max(rounds * tiles, 1), 5)}
                rec.update(_stats(ms))
                rec["voxels_per_s"] = round(vox / (rec["median_ms"] * 1e-3), 1)
                rec.update(extra or {})
                return rec

            ms, reached = _timed(ctx, run, args.warmup, args.steps)
            rec = record("travel_cost_dev", ms, reached)
            # the other whole-grid traversal, same grid, same run (the labels go where toward went)
            cc_ms, components = _timed(ctx, lambda: ctx.connected_components_dev(occ_dev.data_ptr(), shape,
                                                                                  toward.data_ptr()),
                                       args.warmup, args.steps)
            rec["connected_components_median_ms"] = _stats(cc_ms)["median_ms"]
            rec["components"] = components
            rec["travel_over_connected_components"] = round(rec["median_ms"] / rec["connected_components_median_ms"], 2)
            emit(rec)
            full_ms = rec["median_ms"]

            # a limit that reaches about a tenth of the grid
            run()
            reached_costs = cost.view(-1)
            reached_costs = reached_costs[reached_costs != -1]
            limit = int(torch.kthvalue(reached_costs.to(torch.int64), max(1, vox // 10)).values) \
                if reached_costs.numel() > vox // 10 else capi.TRAVEL_NO_LIMIT
            del reached_costs
            ms, reached = _timed(ctx, lambda: run(limit=limit), args.warmup, args.steps)
            emit(record("travel_cost_dev_limited", ms, reached,
                        {"cost_limit": limit, "share_reached": round(reached / vox, 4),
                         "over_unlimited": round(float(np.median(ms)) / full_ms, 3)}))

            if size == max(args.sizes):
                # the SDF threshold form on the grid's own distance field: the map inflated by two cells
                sdf_dev = torch.empty(shape, dtype=torch.float32, device="cuda")
                sdf_ws_bytes = capi.sdf_workspace_bytes(shape)
                sdf_ws = torch.empty(sdf_ws_bytes, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                ctx.sdf_dev(occ_dev.data_ptr(), shape, args.resolution, sdf_dev.data_ptr(), sdf_ws.data_ptr(), sdf_ws_bytes)
                ctx.synchronize()
                del sdf_ws
                threshold = 2.0 * args.resolution
                far = int(torch.argmax(sdf_dev.view(-1)))
                src_dev.fill_(far)
                ms, reached = _timed(ctx, lambda: run(field=sdf_dev, mode=capi.TRAVEL_SDF_ABOVE, threshold=threshold),
                                     args.warmup, args.steps)
                rec = record("travel_cost_dev_sdf_above", ms, reached, {"threshold": threshold})
                rec["source"] = far
                emit(rec)
                src_dev.fill_(source)
                del sdf_dev

            if size == min(args.sizes) and args.paths > 0:
                run()
                reached_cells = torch.nonzero(cost.view(-1) != -1).view(-1).to(torch.int32)
                pick = torch.randint(0, reached_cells.numel(), (args.paths,), device="cuda",
                                     generator=torch.Generator(device="cuda").manual_seed(7))
                starts = reached_cells[pick].contiguous()
                max_cells = 256
                paths = torch.empty((args.paths, max_cells), dtype=torch.int32, device="cuda")
                lengths = torch.empty(args.paths, dtype=torch.int32, device="cuda")
                status = torch.empty(args.paths, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                ms, _ = _timed(ctx, lambda: ctx.trace_paths_dev(toward.data_ptr(), vox, starts.data_ptr(), args.paths,
                                                                max_cells, paths.data_ptr(), lengths.data_ptr(),
                                                                status.data_ptr()), args.warmup, args.steps)
                # (toward was overwritten by the labels above and rebuilt by the run() just before)
                rec = {"case": "trace_paths_dev", "dist": dist, "shape": list(shape), "paths": args.paths,
                       "max_cells": max_cells, "mean_length": round(float(lengths.float().mean()), 2),
                       "ok": int((status == 0).sum()), "truncated": int((status == 2).sum())}
                rec.update(_stats(ms))
                rec["paths_per_s"] = round(args.paths / (rec["median_ms"] * 1e-3), 1)
                emit(rec)
                del paths, lengths, status, starts, reached_cells, pick
            del occ_dev, cost, toward, ws

            if size == args.heap_size:
                import travel_ref
                host_ms, got = _timed(ctx, lambda: ctx.travel_cost(occ_host, [source], weights), 1, 3)
                t0 = time.perf_counter()
                want = travel_ref.dijkstra(travel_ref.passable(occ_host), weights, 0, [source])
                heap_ms = (time.perf_counter() - t0) * 1e3
                rec = {"case": "travel_cost_host_vs_heap", "dist": dist, "shape": list(shape), "heap_ms": round(heap_ms, 1),
                       "heap_equals_device": bool(np.array_equal(want, got[0]))}
                rec.update(_stats(host_ms, "host_"))
                rec["heap_over_host"] = round(heap_ms / rec["host_median_ms"], 1)
                emit(rec)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
