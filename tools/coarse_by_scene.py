#!/usr/bin/env python3
"""The X pass's two kernels by scene (csrc/edt_sweep_kernels.hip, kCoarse), interleaved on one box: per-kernel ms of
device-resident extractions through the testing library with the coarse-hull kernel forced (mode 1), never (mode 2) and
by scene (mode 0), the share of one-class Z lines that pass 1 counts, and the kernel mode 0 chose.
Usage: python tools/coarse_by_scene.py [--reps R] [--calls C] SCENE@NX,NY,NZ ...   (SCENE: spheres, unknown_mix, salt:P)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from voxelized_geometry_tools_amd import capi

CHOICES = {1: "plain (one launch)", 2: "coarse (one launch)", 5: "plain (device)", 6: "coarse (device)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("cases", nargs="+")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0, testing=True)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    for case in args.cases:
        scene, extents = case.split("@")
        shape = tuple(int(v) for v in extents.split(","))
        dist, _, p = scene.partition(":")
        occ = bench.device_occupancy(torch, shape, dist, 42, dev, salt_p=float(p or 0.01))
        # lines along Z that hold one class, as pass 1 counts them
        filled = occ >= 0.5
        share = float((filled.all(dim=2) | ~filled.any(dim=2)).float().mean())
        del filled
        sdf = torch.empty(shape, dtype=torch.float32, device=dev)
        nbytes = capi.sdf_workspace_bytes(shape)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rows = {0: [], 1: [], 2: []}
        chosen = {}
        ref = None
        for _ in range(args.reps):
            for mode in (2, 1, 0):
                ctx.set_coarse_hull(mode)
                for _ in range(2):
                    ctx.sdf_dev(occ.data_ptr(), shape, 0.01, sdf.data_ptr(), ws.data_ptr(), nbytes, None)
                torch.cuda.synchronize()
                ctx.timing_start(args.calls)
                for _ in range(args.calls):
                    ctx.sdf_dev(occ.data_ptr(), shape, 0.01, sdf.data_ptr(), ws.data_ptr(), nbytes, None)
                torch.cuda.synchronize()
                rows[mode].append(ctx.timing_stop().mean(axis=0))
                chosen[mode] = ctx.x_pass_choice(ws.data_ptr(), shape)
                counted = ctx.one_class_counts(ws.data_ptr(), shape)
                if ref is None:
                    ref = sdf.clone()
                else:
                    assert torch.equal(ref.view(torch.int32), sdf.view(torch.int32)), (case, mode)
        ctx.set_coarse_hull(0)
        for mode in (2, 1, 0):
            k = np.array(rows[mode])
            x = k[:, 2]
            print("%-22s one-class lines %.4f (pass 1's sample: %d of %d = %.4f)  mode %d  p1 %.4f  Y %.4f  X %.4f - %.4f (median %.4f)  ran: %s" % (
                case, share, counted[0], counted[1], counted[0] / max(counted[1], 1), mode, np.median(k[:, 0]), np.median(k[:, 1]), x.min(), x.max(), np.median(x),
                CHOICES.get(chosen[mode], chosen[mode])), flush=True)
        del occ, sdf, ws, ref


if __name__ == "__main__":
    main()
