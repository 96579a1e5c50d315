// Segment queries for gfx950: a batch of segments a -> b cast through a float occupancy map or a float SDF, one lane
// per segment.  Semantics, outputs and the one divergence from the reference's walk: include/vgt_hip.h,
// vgt_hip_cast_segments.
//
// The cells.  A segment examines the cells the reference's f64 voxelizer walk (cpu_pointcloud_voxelization.cpp:208-436;
// RaycastKernel<double> in voxelizer_kernels.hip, raycast_one_f64 in the oracle) visits for origin a, point b and an
// unlimited range: the in-grid cells of the walk in walk order, then the final cell.  The set-up below is that kernel's,
// line for line, with max_range = +infinity folded in (nothing is clipped, and `t2 > tmax` / `tmin > tmax` of the slab
// test never hold); this translation unit is built with the same floating-point flags (no contraction, correctly rounded
// division and sqrt), so both walk the same cells bit for bit.
//
// The walk is read-only and its cell sequence does not depend on what it reads: only where it stops does.  So the
// sequence is PRODUCED kLoadAhead cells ahead of where it is EXAMINED: the next cell's step is computed, and its load is
// in flight, while the examined one is tested.  Deeper queues were measured and did not pay (see kLoadAhead).
//
// Two properties the kernel has by construction:
//   bounded   the producer yields at most `total` walk cells, total <= lim0 + lim1 + lim2 + 1 < nx + ny + nz, and
//             `total` is the trip count of its loop; the consumer's loop runs at most total + 1 times.  No value of t or
//             dt (NaN, infinite) and no saturated index can make a lane spin.
//   in bounds every address loaded is a cell the walk examines if nothing stops it earlier: a cell reached by steps
//             that each had lim > 0 from an in-grid start, or the final cell after InGrid(end).  Once the producer is
//             exhausted it repeats the last such cell (cell 0 of the non-empty grid when there was none).
#include "raycast_walk.hpp"
#include "vgt_internal.hpp"

#include <cmath>

// Cells produced (and loads in flight) ahead of the examined one.  Measured at 1, 2, 4 and 8 (DESIGN.md, 4f;
// profiles/segments/ab/): the depth moves the times by a few per cent on scattered segments and costs 17 - 37 % on a depth
// image, so the shipped depth is 1; the A/B builds of tools/ab_segments.sh set it from the command line.
#ifndef VGT_SEGMENT_LOAD_AHEAD
#define VGT_SEGMENT_LOAD_AHEAD 1
#endif

namespace vgt
{
namespace
{
constexpr int kLoadAhead = VGT_SEGMENT_LOAD_AHEAD;
static_assert(kLoadAhead >= 1 && kLoadAhead <= 8, "load-ahead depth");
constexpr int kSegmentThreads = 256;
constexpr uint8_t kSegmentClear = 0, kSegmentHit = 1, kSegmentMissedGrid = 2, kSegmentInvalid = 3;

// The counter of the chosen axis.  (By value: a conditional expression over the variables themselves is an lvalue, and a
// select between their addresses keeps them in memory.)
__device__ __forceinline__ uint32_t OfAxis(bool ax, bool ay, uint32_t x, uint32_t y, uint32_t z)
{
  return ax ? x : (ay ? y : z);
}

template <int kMode>
__device__ __forceinline__ bool IsHit(float value, int unknown_is_filled, double threshold)
{
  if constexpr (kMode == 0)
    return value > 0.5f || (unknown_is_filled && value == 0.5f);
  else
    return static_cast<double>(value) <= threshold;
}

template <int kMode, bool kMin>
__global__ __launch_bounds__(kSegmentThreads) void CastSegmentsKernel(const float* __restrict__ field, const SegmentGrid g,
                                                                     const SegmentQuery q,
                                                                     const double* __restrict__ segments,
                                                                     int64_t num_segments, const SegmentOutputs out)
{
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kSegmentThreads + threadIdx.x;
  if (i >= num_segments) return;
  const double pax = segments[6 * i + 0], pay = segments[6 * i + 1], paz = segments[6 * i + 2];
  const double pbx = segments[6 * i + 3], pby = segments[6 * i + 4], pbz = segments[6 * i + 5];
  const bool valid = isfinite(pax) && isfinite(pay) && isfinite(paz) && isfinite(pbx) && isfinite(pby) && isfinite(pbz);

  // both ends in the grid frame
  double origin[3] = {pax, pay, paz}, last[3] = {pbx, pby, pbz};
  if (g.has_xform)
  {
    const double* T = g.xform;
#pragma unroll
    for (int a = 0; a < 3; a++)
    {
      origin[a] = T[a] * pax + T[4 + a] * pay + T[8 + a] * paz + T[12 + a];
      last[a] = T[a] * pbx + T[4 + a] * pby + T[8 + a] * pbz + T[12 + a];
    }
  }
  const double ray[3] = {last[0] - origin[0], last[1] - origin[1], last[2] - origin[2]};

  // The cell sequence: the walk's counters (as RaycastKernel keeps them) and the final cell.  (Plain locals, not members
  // of one object: the selects between the per-axis counters must stay selects between registers.)
  uint32_t cell = 0;                            // the next walk cell; afterwards the last cell yielded
  uint32_t delta0 = 0, delta1 = 0, delta2 = 0;  // two's complement: cell + delta wraps to the right index
  uint32_t lim0 = 0, lim1 = 0, lim2 = 0;
  uint32_t total = 0;  // walk cells still to yield, at most
  double t0 = 0.0, t1 = 0.0, t2 = 0.0, dt0 = 0.0, dt1 = 0.0, dt2 = 0.0;
  uint32_t end_cell = 0;
  bool end_pending = false;  // the final cell is in the grid and not yet yielded
  if (valid)
  {
    const double length = sqrt(ray[0] * ray[0] + ray[1] * ray[1] + ray[2] * ray[2]);
    // entry point: the origin itself, or where the ray enters the grid's box
    int32_t origin_idx[3];
#pragma unroll
    for (int a = 0; a < 3; a++) origin_idx[a] = RaycastTraits<double>::ToIndex(floor(origin[a] * g.inverse_voxel_size));
    double first[3] = {origin[0], origin[1], origin[2]};
    bool walking = true;
    if (!InGrid(origin_idx, g.counts))
    {
      double tmin = 0.0;
      double dir[3];
#pragma unroll
      for (int a = 0; a < 3; a++) dir[a] = ray[a] / length;
#pragma unroll
      for (int a = 0; a < 3; a++)
      {
        if (fabs(dir[a]) < RaycastTraits<double>::kFlat)
        {
          if (!(origin[a] >= 0.0 && origin[a] < g.grid_size[a])) walking = false;
        }
        else
        {
          const double ood = 1.0 / dir[a];
          const double tlow = (0.0 - origin[a]) * ood;
          const double thigh = (g.grid_size[a] - origin[a]) * ood;
          const double t1 = (tlow <= thigh) ? tlow : thigh;
          if (t1 > tmin) tmin = t1;
        }
      }
      // the stated divergence: the segment ends before it reaches the grid (also: length zero, direction 0 / 0)
      if (tmin + RaycastTraits<double>::kNudge > length) walking = false;
#pragma unroll
      for (int a = 0; a < 3; a++) first[a] = origin[a] + (dir[a] * (tmin + RaycastTraits<double>::kNudge));
    }
    if (walking)
    {
      const double half = g.voxel_size * 0.5;
      int32_t cur[3], end[3];
      double t[3], dt[3];
      uint32_t lim[3];
      int64_t move[3];
      uint64_t remaining = 0;
      const int64_t stride[3] = {static_cast<int64_t>(g.counts[1]) * g.counts[2], g.counts[2], 1};
#pragma unroll
      for (int a = 0; a < 3; a++)
      {
        cur[a] = RaycastTraits<double>::ToIndex(floor(first[a] * g.inverse_voxel_size));
        end[a] = RaycastTraits<double>::ToIndex(floor(last[a] * g.inverse_voxel_size));
        const int64_t diff = static_cast<int64_t>(end[a]) - cur[a];
        const int32_t step = (diff > 0) - (diff < 0);
        const double centre = (static_cast<double>(cur[a]) + 0.5) * g.voxel_size;
        t[a] = AxisT<double>(first[a], ray[a], centre - half, centre + half);
        dt[a] = fabs(g.voxel_size / ray[a]);
        const uint64_t apart = static_cast<uint64_t>(diff < 0 ? -diff : diff);  // < 2^32
        remaining += apart;
        // (meaningful only when cur is inside the grid, which is tested below)
        const uint32_t room = static_cast<uint32_t>(step > 0 ? g.counts[a] - 1 - cur[a] : cur[a]);
        lim[a] = static_cast<uint32_t>(apart < room ? apart : room);
        move[a] = step * stride[a];
      }
      if (InGrid(end, g.counts))
      {
        end_cell = static_cast<uint32_t>(CellIndex(end, g.counts));
        end_pending = true;
      }
      if (remaining != 0 && InGrid(cur, g.counts))
      {
        // every step but the last takes one off a lim: the walk yields at most lim0 + lim1 + lim2 + 1 cells
        const uint64_t most = static_cast<uint64_t>(lim[0]) + lim[1] + lim[2] + 1u;
        total = static_cast<uint32_t>(remaining < most ? remaining : most);
        cell = static_cast<uint32_t>(CellIndex(cur, g.counts));
        delta0 = static_cast<uint32_t>(move[0]);
        delta1 = static_cast<uint32_t>(move[1]);
        delta2 = static_cast<uint32_t>(move[2]);
        lim0 = lim[0], lim1 = lim[1], lim2 = lim[2];
        t0 = t[0], t1 = t[1], t2 = t[2];
        dt0 = dt[0], dt1 = dt[1], dt2 = dt[2];
      }
    }
  }

  // -> whether there was another cell; `next` is always a cell whose load is in bounds (see the header).
  auto next_cell = [&](uint32_t& next) -> bool {
    if (total != 0u)
    {
      next = cell;
      // the axis whose boundary comes first: X if t.x is the least or tied least, else Y if t.y is, else Z
      const bool ax = (t0 <= t1) & (t0 <= t2);
      const bool ay = !ax & (t1 <= t0) & (t1 <= t2);
      const bool az = !(ax | ay);
      const uint32_t lim = OfAxis(ax, ay, lim0, lim1, lim2);
      lim0 -= ax ? 1u : 0u;
      lim1 -= ay ? 1u : 0u;
      lim2 -= az ? 1u : 0u;
      t0 = ax ? t0 + dt0 : t0;
      t1 = ay ? t1 + dt1 : t1;
      t2 = az ? t2 + dt2 : t2;
      total -= 1u;
      // lim == 0: cur[a] == end[a] (the reference's break) or the step leaves the grid -- the walk ends at `next`, and
      // `cell` stays on it, so that it never holds an index past a lim of 0
      if (lim == 0u) total = 0u;
      if (total != 0u) cell += OfAxis(ax, ay, delta0, delta1, delta2);
      return true;
    }
    const bool more = end_pending;
    if (more) cell = end_cell;
    end_pending = false;
    next = cell;
    return more;
  };

  // Examination, kLoadAhead cells behind the producer.
  const bool walk_through = (q.flags & 1u) != 0u;
  const uint32_t most_examined = total + (end_pending ? 1u : 0u);
  uint32_t queued_cell[kLoadAhead];
  float queued_value[kLoadAhead];
  bool queued[kLoadAhead];
#pragma unroll
  for (int k = 0; k < kLoadAhead; k++)
  {
    queued[k] = next_cell(queued_cell[k]);
    queued_value[k] = field[queued_cell[k]];
  }
  int32_t hit_index = -1, examined = 0, min_index = -1;
  float min_value = NAN;
  for (uint32_t k = 0; k < most_examined; k++)
  {
    if (!queued[0]) break;
    const uint32_t here = queued_cell[0];
    const float value = queued_value[0];
    examined++;
    if constexpr (kMin)
    {
      if (!isnan(value) && (min_index < 0 || value < min_value))
      {
        min_value = value;
        min_index = static_cast<int32_t>(here);
      }
    }
    if (hit_index < 0 && IsHit<kMode>(value, q.unknown_is_filled, q.threshold))
    {
      hit_index = static_cast<int32_t>(here);
      if (!walk_through) break;
    }
#pragma unroll
    for (int j = 0; j + 1 < kLoadAhead; j++)
    {
      queued[j] = queued[j + 1];
      queued_cell[j] = queued_cell[j + 1];
      queued_value[j] = queued_value[j + 1];
    }
    queued[kLoadAhead - 1] = next_cell(queued_cell[kLoadAhead - 1]);
    queued_value[kLoadAhead - 1] = field[queued_cell[kLoadAhead - 1]];
  }

  out.status_dev[i] = !valid ? kSegmentInvalid
                         : (hit_index >= 0 ? kSegmentHit : (examined > 0 ? kSegmentClear : kSegmentMissedGrid));
  if (out.hit_index_dev) out.hit_index_dev[i] = hit_index;
  if (out.cells_examined_dev) out.cells_examined_dev[i] = examined;
  if (out.hit_fraction_dev)
  {
    double fraction = NAN;
    if (hit_index >= 0)
    {
      const int32_t plane = g.counts[1] * g.counts[2];
      const int32_t x = hit_index / plane, rest = hit_index - x * plane;
      const int32_t y = rest / g.counts[2];
      const int32_t idx[3] = {x, y, rest - y * g.counts[2]};
      double enter = 0.0;
#pragma unroll
      for (int a = 0; a < 3; a++)
      {
        if (ray[a] != 0.0)
        {
          const double lo = static_cast<double>(idx[a]) * g.voxel_size;
          const double hi = static_cast<double>(idx[a] + 1) * g.voxel_size;
          const double ta = (lo - origin[a]) / ray[a], tb = (hi - origin[a]) / ray[a];
          const double m = ta < tb ? ta : tb;
          if (m > enter) enter = m;
        }
      }
      fraction = enter > 1.0 ? 1.0 : enter;
    }
    out.hit_fraction_dev[i] = fraction;
  }
  if constexpr (kMin)
  {
    if (out.min_value_dev) out.min_value_dev[i] = min_value;
    if (out.min_index_dev) out.min_index_dev[i] = min_index;
  }
}
}  // namespace

hipError_t LaunchCastSegments(const float* field_dev, const SegmentGrid& grid, const SegmentQuery& query,
                              const double* segments_dev, int64_t num_segments, const SegmentOutputs& out,
                              hipStream_t stream)
{
  if (num_segments <= 0) return hipSuccess;
  const dim3 blocks(static_cast<unsigned>((num_segments + kSegmentThreads - 1) / kSegmentThreads));
  const dim3 threads(kSegmentThreads);
  const bool with_min = out.min_value_dev || out.min_index_dev;
  if (query.mode == kSegmentOccupancy)
    hipLaunchKernelGGL((CastSegmentsKernel<0, false>), blocks, threads, 0, stream, field_dev, grid, query, segments_dev,
                       num_segments, out);
  else if (with_min)
    hipLaunchKernelGGL((CastSegmentsKernel<1, true>), blocks, threads, 0, stream, field_dev, grid, query, segments_dev,
                       num_segments, out);
  else
    hipLaunchKernelGGL((CastSegmentsKernel<1, false>), blocks, threads, 0, stream, field_dev, grid, query, segments_dev,
                       num_segments, out);
  return hipGetLastError();
}
}  // namespace vgt
