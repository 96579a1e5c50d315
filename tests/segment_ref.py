"""CPU restatement of vgt_hip_cast_segments (include/vgt_hip.h): the ordered cells a segment examines -- the reference's
f64 voxelizer walk (cpu_pointcloud_voxelization.cpp:208-436, the oracle's raycast_one_f64) for origin A, point B and
max_range = +infinity, in its (cur, end, step) form, in-grid walk cells first and the final cell last --, the predicate,
and the six outputs.  Plain Python over numpy float64 scalars: IEEE double, one operation at a time, no contraction.
tests/test_segment_ref.py pins it against the oracle's walk and against geometry before anything trusts it."""
import collections
import math

import numpy as np

OCCUPANCY, SDF_BELOW = 0, 1
CLEAR, HIT, MISSED_GRID, INVALID = 0, 1, 2, 3
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
FLAT = 1e-10
NUDGE = 1e-10

f64 = np.float64

Casts = collections.namedtuple("Casts", "status hit_index hit_fraction cells_examined min_value min_index")
# cells: the ordered list of (x, y, z); ended_before: the origin is outside the grid and tmin + 1e-10 > length (the
# divergence rule then drops the segment); ended_short: the walk left through its `cur[a] == end[a]` break
Walk = collections.namedtuple("Walk", "cells ended_before ended_short")


def to_index(floored):
    """RaycastTraits<double>::ToIndex: the CPU voxelizer's cast, saturated to int32."""
    if not (floored > -9223372036854775808.0 and floored < 9223372036854775808.0):
        return INT32_MIN
    if floored >= 2147483648.0:
        return INT32_MAX
    if floored <= -2147483648.0:
        return INT32_MIN
    return int(floored)


def in_grid(idx, counts):
    return all(0 <= idx[a] < counts[a] for a in range(3))


def axis_t(point, ray, lo, hi):
    if ray > 0.0:
        return abs((hi - point) / ray)
    if ray < -0.0:
        return abs((point - lo) / ray)
    return f64(math.inf)


def transform(xform, p):
    """X p, 16 doubles column-major, each row as ((m0*x + m4*y) + m8*z) + m12; None = p as it is."""
    p = [f64(c) for c in p]
    if xform is None:
        return p
    m = [f64(v) for v in np.asarray(xform, dtype=np.float64).reshape(16)]
    return [((m[r] * p[0] + m[4 + r] * p[1]) + m[8 + r] * p[2]) + m[12 + r] for r in range(3)]


def walk(A, B, counts, resolution, divergence=True):
    """The cells the segment A -> B (grid frame, finite) examines, in order.  divergence=False: the reference's walk
    as it is, without the rule that drops segments that end before the grid."""
    with np.errstate(all="ignore"):
        A, B = [f64(c) for c in A], [f64(c) for c in B]
        vs = f64(resolution)
        ivs = f64(1.0) / vs
        grid_size = [f64(counts[a]) * vs for a in range(3)]
        ray = [B[a] - A[a] for a in range(3)]
        length = np.sqrt((ray[0] * ray[0] + ray[1] * ray[1]) + ray[2] * ray[2])
        origin_idx = [to_index(np.floor(A[a] * ivs)) for a in range(3)]
        first = list(A)
        ended_before = False
        if not in_grid(origin_idx, counts):
            tmin, tmax = f64(0.0), f64(math.inf)
            direction = [ray[a] / length for a in range(3)]
            for a in range(3):
                if abs(direction[a]) < FLAT:
                    if not (A[a] >= 0.0 and A[a] < grid_size[a]):
                        return Walk([], False, False)
                else:
                    ood = f64(1.0) / direction[a]
                    tlow = (f64(0.0) - A[a]) * ood
                    thigh = (grid_size[a] - A[a]) * ood
                    t1 = tlow if tlow <= thigh else thigh
                    t2 = thigh if tlow <= thigh else tlow
                    if t1 > tmin:
                        tmin = t1
                    if t2 > tmax:  # as the reference
                        tmax = t2
                    if tmin > tmax:
                        return Walk([], False, False)
            ended_before = bool(tmin + f64(NUDGE) > length)
            if ended_before and divergence:
                return Walk([], True, False)
            first = [A[a] + (direction[a] * (tmin + f64(NUDGE))) for a in range(3)]
        cur = [to_index(np.floor(first[a] * ivs)) for a in range(3)]
        end = [to_index(np.floor(B[a] * ivs)) for a in range(3)]
        step = [(end[a] > cur[a]) - (end[a] < cur[a]) for a in range(3)]
        half = vs * f64(0.5)
        t, dt = [], []
        for a in range(3):
            centre = (f64(cur[a]) + f64(0.5)) * vs
            t.append(axis_t(first[a], ray[a], centre - half, centre + half))
            dt.append(abs(vs / ray[a]))
        cells, ended_short = [], False
        c = list(cur)
        while c != end:
            if not in_grid(c, counts):
                break
            cells.append(tuple(c))
            if t[0] <= t[1] and t[0] <= t[2]:
                a = 0
            elif t[1] <= t[0] and t[1] <= t[2]:
                a = 1
            else:
                a = 2
            if c[a] == end[a]:
                ended_short = True
                break
            c[a] += step[a]
            t[a] = t[a] + dt[a]
        if in_grid(end, counts):
            cells.append(tuple(end))
        return Walk(cells, ended_before, ended_short)


def is_hit(value, mode, unknown_is_filled, threshold):
    value = np.float32(value)
    if mode == OCCUPANCY:
        return bool(value > np.float32(0.5) or (unknown_is_filled and value == np.float32(0.5)))
    return bool(f64(value) <= f64(threshold))


def hit_fraction(A, B, idx, resolution):
    with np.errstate(all="ignore"):
        vs = f64(resolution)
        enter = f64(0.0)
        for a in range(3):
            d = f64(B[a]) - f64(A[a])
            if d != 0.0:
                lo, hi = f64(idx[a]) * vs, f64(idx[a] + 1) * vs
                ta, tb = (lo - f64(A[a])) / d, (hi - f64(A[a])) / d
                m = ta if ta < tb else tb
                if m > enter:
                    enter = m
        return f64(1.0) if enter > 1.0 else enter


def walks(counts, resolution, segments, grid_from_world=None):
    """Per segment None (a coordinate is not finite) or (A, B, cells): the part of cast() that does not depend on the
    field, for callers that cast the same segments more than once."""
    out = []
    for s in np.asarray(segments, dtype=np.float64).reshape(-1, 6):
        if not np.all(np.isfinite(s)):
            out.append(None)
            continue
        A, B = transform(grid_from_world, s[:3]), transform(grid_from_world, s[3:])
        out.append((A, B, walk(A, B, counts, resolution).cells))
    return out


def cast(field, resolution, segments, mode=OCCUPANCY, unknown_is_filled=True, threshold=0.0, walk_through=False,
         grid_from_world=None, with_min=False, walked=None):
    """-> Casts of arrays with the dtypes of the C ABI; min_value / min_index are None unless with_min.  walked: what
    walks() gave for the same grid, segments and frame."""
    field = np.asarray(field, dtype=np.float32)
    counts = field.shape
    seg = np.asarray(segments, dtype=np.float64).reshape(-1, 6)
    n = len(seg)
    status = np.empty(n, dtype=np.uint8)
    hit_index = np.full(n, -1, dtype=np.int32)
    fraction = np.full(n, np.nan, dtype=np.float64)
    examined = np.zeros(n, dtype=np.int32)
    min_value = np.full(n, np.nan, dtype=np.float32)
    min_index = np.full(n, -1, dtype=np.int32)
    if walked is None:
        walked = walks(counts, resolution, seg, grid_from_world)
    for i in range(n):
        if walked[i] is None:
            status[i] = INVALID
            continue
        A, B, cells = walked[i]
        for cell in cells:
            value = field[cell]
            index = (cell[0] * counts[1] + cell[1]) * counts[2] + cell[2]
            examined[i] += 1
            if not np.isnan(value) and (min_index[i] < 0 or value < min_value[i]):
                min_value[i], min_index[i] = value, index
            if hit_index[i] < 0 and is_hit(value, mode, unknown_is_filled, threshold):
                hit_index[i] = index
                fraction[i] = hit_fraction(A, B, cell, resolution)
                if not walk_through:
                    break
        status[i] = HIT if hit_index[i] >= 0 else (CLEAR if examined[i] > 0 else MISSED_GRID)
    if not with_min:
        min_value = min_index = None
    return Casts(status, hit_index, fraction, examined, min_value, min_index)
