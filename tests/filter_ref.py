"""CPU yardstick of the voxelizer's combine-and-filter step (beside fill_ref.py; not a test module).

The reference's rule restated in vectorised numpy from the reference's own source -- not from FilterKernel, and without
calling the oracle library (tests/test_filter_ref.py compares the two):

  device rule   S/cuda_voxelization_helpers.cu:358-426 (FilterGrids), the threshold cast to float once by its caller,
                S/device_pointcloud_voxelization.cpp:155-156
  double rule   I/pointcloud_voxelization_interface.hpp:55-86 (CountsSeenAs) inside
                S/cpu_pointcloud_voxelization.cpp:438-490 (DoCombineAndFilterGrids)

Per cell whose static occupancy is `<= 0.5` (cuda_voxelization_helpers.cu:371, cpu_pointcloud_voxelization.cpp:453), and
per tracking grid ("camera"):
  filtered_filled = filled if filled >= outlier_points_threshold else 0            (.cu:384-385, .hpp:58-59)
  free > 0 and filtered_filled > 0:  ratio = free / (free + filtered_filled), the sum taken in int32 first and both
                                     operands then converted to the ratio's type (.cu:388-390 float, .hpp:62-64 double);
                                     ratio >= percent_seen_free -> the camera saw free, otherwise filled (.cu:391, .hpp:65)
  free > 0 alone -> free; filtered_filled > 0 alone -> filled; neither -> the camera says nothing      (.cu:400-407)
then  any camera filled -> 1.0;  else free cameras >= num_cameras_seen_free -> 0.0;  else 0.5          (.cu:409-423)

Every other cell keeps its value bit for bit.  A static occupancy of NaN: `current_occupancy <= 0.5f`
(S/cuda_voxelization_helpers.cu:371; `current_cell.Occupancy() <= 0.5` in S/cpu_pointcloud_voxelization.cpp:453) is
false for NaN, so the reference never enters the block and a NaN cell is SKIPPED like a filled one, payload and sign
untouched.  The rule is therefore "not (occupancy <= 0.5)", which is not the same as "occupancy > 0.5".

`free + filled` overflowing int32 is undefined in the reference; callers keep counts below 2^30.
"""
import numpy as np


def seen_as(free, filled, percent_seen_free, outlier_points_threshold, ratio_in_double, strict=False):
    """Per camera and cell: (saw_free, saw_filled) bool arrays.  `strict` replaces the rule's `>=` on the ratio by `>`:
    not the reference's rule, only there so that a test can show which cells are exact ties."""
    free = np.asarray(free, dtype=np.int32)
    filled = np.asarray(filled, dtype=np.int32)
    filtered = np.where(filled >= np.int32(outlier_points_threshold), filled, np.int32(0)).astype(np.int32)
    both = (free > 0) & (filtered > 0)
    total = (free + filtered).astype(np.int32)
    assert (total >= 0).all(), "free + filled overflowed int32: out of the rule's scope"
    real = np.float64 if ratio_in_double else np.float32
    threshold = real(percent_seen_free)
    denominator = np.where(both, total, np.int32(1)).astype(real)
    ratio = free.astype(real) / denominator
    assert ratio.dtype == real
    passes = (ratio > threshold) if strict else (ratio >= threshold)
    saw_free = (both & passes) | (~both & (free > 0))
    saw_filled = (both & ~passes) | (~both & (filtered > 0))
    return saw_free, saw_filled


def filter_grids(tracking, occupancy, percent_seen_free=1.0, outlier_points_threshold=1, num_cameras_seen_free=1,
                 ratio_in_double=False, strict=False):
    """tracking int32 [grids, ..., 2] = (seen free, seen filled) per camera; occupancy float32 [...] -> filtered copy."""
    tracking = np.asarray(tracking, dtype=np.int32)
    occupancy = np.asarray(occupancy, dtype=np.float32)
    assert tracking.shape[1:] == occupancy.shape + (2,)
    saw_free, saw_filled = seen_as(tracking[..., 0], tracking[..., 1], percent_seen_free, outlier_points_threshold,
                                   ratio_in_double, strict)
    cameras_free = saw_free.sum(axis=0, dtype=np.int32)
    cameras_filled = saw_filled.sum(axis=0, dtype=np.int32)
    verdict = np.where(cameras_filled > 0, np.float32(1.0),
                       np.where(cameras_free >= np.int32(num_cameras_seen_free), np.float32(0.0), np.float32(0.5)))
    with np.errstate(invalid="ignore"):
        touched = occupancy <= np.float32(0.5)
    out = occupancy.copy()
    out[touched] = verdict.astype(np.float32)[touched]
    return out


def skipped(occupancy):
    """bool: the cells the filter leaves alone."""
    with np.errstate(invalid="ignore"):
        return ~(np.asarray(occupancy, dtype=np.float32) <= np.float32(0.5))
