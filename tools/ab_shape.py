#!/usr/bin/env python3
"""Per-kernel ms of device-resident SDF extractions of one library (VGT_HIP_LIB) on a grid bench.py has no option for:
python tools/ab_shape.py SCENE@NX,NY,NZ [--calls C]   (SCENE: spheres, unknown_mix, salt:P).  For A / B runs of two builds,
one process each, interleaved by the caller."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from voxelized_geometry_tools_amd import capi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case")
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    scene, extents = args.case.split("@")
    shape = tuple(int(v) for v in extents.split(","))
    dist, _, p = scene.partition(":")
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    occ = bench.device_occupancy(torch, shape, dist, 42, dev, salt_p=float(p or 0.01))
    sdf = torch.empty(shape, dtype=torch.float32, device=dev)
    nbytes = capi.sdf_workspace_bytes(shape)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    for _ in range(5):
        ctx.sdf_dev(occ.data_ptr(), shape, 0.01, sdf.data_ptr(), ws.data_ptr(), nbytes, None)
    torch.cuda.synchronize()
    ctx.timing_start(args.calls)
    for _ in range(args.calls):
        ctx.sdf_dev(occ.data_ptr(), shape, 0.01, sdf.data_ptr(), ws.data_ptr(), nbytes, None)
    torch.cuda.synchronize()
    k = ctx.timing_stop().mean(axis=0)
    print("%-28s %-24s p1 %.4f  Y %.4f  X %.4f  sum %.4f" % (os.path.basename(capi.LIB_PATH), args.case, k[0], k[1], k[2], k.sum()))


if __name__ == "__main__":
    main()
