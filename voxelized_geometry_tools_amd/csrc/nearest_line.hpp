// The per-line routine of the nearest-other-class transform (nearest_kernels.hip; contract: include/vgt_hip.h,
// vgt_hip_nearest_dev): one lower envelope of parabolas along a line of `rows` rows for ONE query class, carrying the
// site (the row it stands on and that row's record) and not only the distance.  __host__ __device__, so that
// tests/cpp/nearest_line_host.cc compiles it with g++ and runs the very code the kernels run -- the routine, and the
// two lines the Y and the X pass hand to it (YLine, XLine below).
//
// Every decision is integer arithmetic: heights are below 2^29, a row offset squared is at most 2^28, so every value
// compared is below 2^30; the boundary between two sites is an exact floor of non-negative integers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "nearest_internal.hpp"

namespace vgt
{
// What the routine asks of a line (`Line`):
//   uint32_t Load(int r) const                        the record of row r
//   bool     IsClass(uint32_t record, int k) const    the row's own cell is of class k
//   int32_t  Height(uint32_t record, int k) const     height of row r as a site for queries of class k: 0 when the
//                                                     row's cell is of the other class, else the squared distance
//                                                     to the row's own nearest other-class cell, or -1: no site
//   void     Emit(int u, int s, uint32_t record_of_s, int k)   row u (of class k) takes the site of row s; s = -1: none
// and of the stack (`Stack`): Put(slot, a, b) / Get(slot, &a, &b) of two 32-bit words, slots 0 .. rows - 2.
//
// Tie rule: among sites at equal distance from a row, the one on the lowest row wins (a site takes over from the one
// below it only where it is strictly nearer).  The result is a pure function of the line.
//
// The hull is Meijster's form of the Felzenszwalb-Huttenlocher envelope: entry j holds its site's row s_j and the
// first row t_j from which it is the nearest of the sites seen so far (t_0 = 0).  The top entry lives in registers;
// entry j < top lives in stack slot j.
// Returns whether the line holds a row of the other class (the caller runs that class's envelope only then); the line
// must hold a row of class k.
template <class Line, class Stack>
__host__ __device__ inline bool NearestLineForClass(int rows, int k, const Line& line, Stack& stack)
{
  int depth = 0;  // entries on the hull
  int top_s = 0, top_t = 0;
  uint32_t top_rec = 0;
  int32_t top_h = 0;
  bool other_class_present = false;
  for (int u = 0; u < rows; u++)
  {
    const uint32_t rec = line.Load(u);
    other_class_present |= !line.IsClass(rec, k);
    const int32_t h = line.Height(rec, k);
    if (h < 0) continue;
    // entries that the new site beats already at their first row are never the nearest: off the hull
    while (depth > 0)
    {
      const int32_t du = top_t - u, ds = top_t - top_s;
      if (ds * ds + top_h <= du * du + h) break;
      depth--;
      if (depth > 0)
      {
        uint32_t a, b;
        stack.Get(depth - 1, &a, &b);
        top_s = static_cast<int>(a & 0xffffu);
        top_t = static_cast<int>(a >> 16);
        top_rec = b;
        top_h = line.Height(b, k);
      }
    }
    int t = 0;
    if (depth > 0)
    {
      // site u is strictly nearer than the top's site s at row x  <=>  2 (u - s) x > (u^2 + h_u) - (s^2 + h_s) =: num,
      // and num >= 2 (u - s) top_t >= 0 because the top survived the loop above: first such row = num / den + 1
      const int32_t num = (u * u + h) - (top_s * top_s + top_h);
      const int32_t den = 2 * (u - top_s);
      t = static_cast<int>(static_cast<uint32_t>(num) / static_cast<uint32_t>(den)) + 1;
      if (t >= rows) continue;  // never the nearest on this line
      stack.Put(depth - 1, static_cast<uint32_t>(top_s) | (static_cast<uint32_t>(top_t) << 16), top_rec);
    }
    depth++;
    top_s = u;
    top_t = t;
    top_rec = rec;
    top_h = h;
  }
  for (int u = rows - 1; u >= 0; u--)
  {
    if (line.IsClass(line.Load(u), k)) line.Emit(u, depth > 0 ? top_s : -1, top_rec, k);
    if (depth > 0 && u == top_t)
    {
      depth--;
      if (depth > 0)
      {
        uint32_t a, b;
        stack.Get(depth - 1, &a, &b);
        top_s = static_cast<int>(a & 0xffffu);
        top_t = static_cast<int>(a >> 16);
        top_rec = b;
      }
    }
  }
  return other_class_present;
}

// Both query classes of a line, one envelope each: the class of row 0 first, the other one only when the line holds it
// (for a line of one class that envelope would have no row to answer, and every row on its hull).
template <class Line, class Stack>
__host__ __device__ inline void NearestLine(int rows, const Line& line, Stack& stack)
{
  const int first = line.IsClass(line.Load(0), 1) ? 1 : 0;
  if (NearestLineForClass(rows, first, line, stack)) NearestLineForClass(rows, 1 - first, line, stack);
}

// --- the two lines of the transform (records: nearest_internal.hpp) ---
__host__ __device__ inline int ClassOf(uint32_t record) { return static_cast<int>((record >> 15) & 1u); }

// The line (x, z) along y: Z records in, Y records out.
struct YLine
{
  const uint16_t* in;  // the line's row 0
  uint32_t* out;
  int64_t stride;  // cells between rows: nz
  int z;
  __host__ __device__ inline uint32_t Load(int r) const { return in[r * stride]; }
  __host__ __device__ inline bool IsClass(uint32_t record, int k) const { return ClassOf(record) == k; }
  __host__ __device__ inline int32_t Height(uint32_t record, int k) const
  {
    if (ClassOf(record) != k) return 0;
    const uint32_t zs = record & kNearestNoneZ;
    if (zs == kNearestNoneZ) return -1;
    const int32_t d = z - static_cast<int32_t>(zs);
    return d * d;
  }
  __host__ __device__ inline void Emit(int u, int s, uint32_t record, int k) const
  {
    uint32_t word = (k ? kNearestFilledBit : 0u) | kNearestNoneZ;
    if (s >= 0)
    {
      const uint32_t zs = ClassOf(record) != k ? static_cast<uint32_t>(z) : (record & kNearestNoneZ);
      word = (static_cast<uint32_t>(s) << 16) | (k ? kNearestFilledBit : 0u) | zs;
    }
    out[u * stride] = word;
  }
};

// The line (y, z) along x: Y records in, linear index and squared distance out.
struct XLine
{
  const uint32_t* in;  // the line's row 0
  int32_t* nearest;
  int32_t* d2;     // or nullptr
  int64_t stride;  // cells between rows: ny * nz
  int32_t nz, y, z;
  __host__ __device__ inline uint32_t Load(int r) const { return in[r * stride]; }
  __host__ __device__ inline bool IsClass(uint32_t record, int k) const { return ClassOf(record) == k; }
  __host__ __device__ inline int32_t Height(uint32_t record, int k) const
  {
    if (ClassOf(record) != k) return 0;
    const uint32_t zs = record & kNearestNoneZ;
    if (zs == kNearestNoneZ) return -1;
    const int32_t dy = y - static_cast<int32_t>(record >> 16), dz = z - static_cast<int32_t>(zs);
    return dy * dy + dz * dz;
  }
  __host__ __device__ inline void Emit(int u, int s, uint32_t record, int k) const
  {
    int32_t index = kNearestNoIndex, distance = kNearestNoDistance;
    if (s >= 0)
    {
      const bool own = ClassOf(record) != k;  // the row's own cell is the site
      const int32_t ty = own ? y : static_cast<int32_t>(record >> 16);
      const int32_t tz = own ? z : static_cast<int32_t>(record & kNearestNoneZ);
      index = static_cast<int32_t>(s * stride + static_cast<int64_t>(ty) * nz + tz);
      distance = (u - s) * (u - s) + Height(record, k);
    }
    nearest[u * stride] = index;
    if (d2) d2[u * stride] = distance;
  }
};
}  // namespace vgt
