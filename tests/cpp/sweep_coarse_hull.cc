// CPU check of the coarse-hull form of the plain X pass (csrc/edt_sweep_kernels.hip, kCoarse, compiled by g++ against
// tests/cpp/hip_shim, lanes one at a time, like sweep_emulation.cc): the line is swept over every 32nd row first, and in the
// sweep proper a row strictly above the chord between the two subsample vertices around it never touches the stack.  Lines of
// 65 to 1024 rows -- two subsample rows, a last band that is partial, a subsample that ends on the last row or before it --
// run with the coarse form on and off against the brute-force line transform, bit for bit, on fields where the filter removes
// most rows (distance-like), none (salt), and on the lines where its bookkeeping could slip: no site at all, a single site at
// row 0 or at the last row, a subsample without any site, inputs at the limit of the 22-bit entries, a plane of one class
// between planes that have sites (three slots here, so a slot's coarse area always holds an earlier item's hull).  Under
// VGT_HOST_EMULATION the kernel records every row with a site that the chord test drops; each of them must be absent from
// the stack that the unfiltered algorithm holds when the line ends.
#ifdef NDEBUG
#error "the kernel's assertions are part of the check: build without NDEBUG"
#endif
#include <hip/hip_runtime.h>

#include <cstdio>
#include <map>
#include <set>
#include <vector>

#define BlockMinMax BlockMinMaxOnDevice
#include "../../voxelized_geometry_tools_amd/csrc/edt_device.hpp"
#undef BlockMinMax
namespace vgt
{
void SetLastError(const std::string&) {}
inline void BlockMinMax(uint32_t lo, uint32_t hi, uint32_t* minmax_enc)
{
  minmax_enc[0] = std::min(minmax_enc[0], lo);
  minmax_enc[1] = std::max(minmax_enc[1], hi);
}
int ShortLineOverride() { return -1; }
}  // namespace vgt
#include "../../voxelized_geometry_tools_amd/csrc/edt_sweep_kernels.hip"

namespace
{
int failures = 0;
uint64_t drops_checked = 0;

int64_t BruteRow(const std::vector<int64_t>& f, const std::vector<uint8_t>& neg, int n, int q)
{
  int64_t best = INT64_MAX;
  for (int r = 0; r < n; r++)
  {
    const int64_t d = static_cast<int64_t>(q - r) * (q - r);
    if (f[r] >= 0) best = std::min(best, d + f[r]);
    if (neg[r] != neg[q]) best = std::min(best, d);
  }
  return best;
}

// Rows on the stack of the Felzenszwalb-Huttenlocher sweep over every site of the line when the line ends, with the
// kernel's pop test and none of its filters (a filter only ever keeps rows off the stack).
std::set<int> ReferenceStack(const std::vector<int64_t>& f, int n)
{
  std::vector<std::pair<int64_t, int>> st;  // (G, row)
  for (int q = 0; q < n; q++)
  {
    if (f[q] < 0) continue;
    const int64_t G = f[q] + static_cast<int64_t>(q) * q;
    while (st.size() >= 2)
    {
      const auto& t = st[st.size() - 1];
      const auto& s = st[st.size() - 2];
      if ((G - t.first) * (t.second - s.second) + (s.first - t.first) * (q - t.second) < 0)
        st.pop_back();
      else
        break;
    }
    st.emplace_back(G, q);
  }
  std::set<int> rows;
  for (const auto& e : st) rows.insert(e.second);
  return rows;
}

// Planes of the grid (y): 0 distance-like, 1 salt, 2 lines without a site / with one at row 0 / at the last row / both,
// 3 a subsample without any site, 4 inputs at the 22-bit limit, 5 distance-like, 6 one class and no site, 7 distance-like.
constexpr int kPlanes = 8;

void Check(int n)
{
  const int nx = n, ny = kPlanes, nz = 70;
  const int64_t total = static_cast<int64_t>(nx) * ny * nz;
  // the largest input the extents allow with 32-bit entries: (nz_global - 1)^2 + (ny - 1)^2 + (n - 1)^2 just below the sentinels
  const int64_t room = vgt::Codec<true>::kSentinelG - 1 - static_cast<int64_t>(n - 1) * (n - 1) - (ny - 1) * (ny - 1);
  int64_t nzg = 1;
  while (nzg * nzg <= room) nzg++;  // (nzg - 1)^2 <= room
  const int64_t max_f = (nzg - 1) * (nzg - 1) + (ny - 1) * (ny - 1);
  std::vector<int32_t> in(total);
  for (int y = 0; y < ny; y++)
    for (int z = 0; z < nz; z++)
      for (int x = 0; x < nx; x++)
      {
        int64_t v = -1;  // no site
        uint8_t cls = static_cast<uint8_t>((x / 23 + z / 5 + y) & 1);
        switch (y)
        {
          case 0:
          case 5:
          case 7:
          {
            // the squared distance to the nearest of a few sites of the line's plane, each (x - sx)^2 / 3 + offset: smooth,
            // locally convex, its rows popped by sites far away -- what the X pass meets on a sparse scene
            v = INT64_MAX;
            // (short lines: two steep sites, so that the kink between them rises above a chord of 32 rows)
            const bool steep = nx < 512;
            for (int site = 0; site < (steep ? 2 : 5); site++)
            {
              const int64_t sx = (static_cast<int64_t>(y) * 7919 + z * 104729 + site * 31337) % nx;
              const int64_t offset = ((y * 13 + z * 7 + site * 101) % 97) * (static_cast<int64_t>(nx) * nx / 300 + 1);
              v = std::min(v, (steep ? (x - sx) * (x - sx) * 3 : (x - sx) * (x - sx) / 3) + offset + 1);
            }
            if ((x + 3 * z) % 11 == 0) v = -1;  // (and some rows that are no site)
            break;
          }
          case 1: v = 1 + static_cast<int64_t>((x * 2654435761ull + z * 40503ull) % 4294967291ull % 50ull); break;
          case 2:
            cls = static_cast<uint8_t>(z & 1);
            if ((z % 4 == 1 || z % 4 == 3) && x == 0) v = 5 + z;
            if ((z % 4 == 2 || z % 4 == 3) && x == nx - 1) v = 7 + z;
            break;
          case 3: v = (x % 32 == 0) ? -1 : 1 + (static_cast<int64_t>(x - nx / 2) * (x - nx / 2) / 2 + z * 17) % 20000; break;
          case 4: v = (x % 37 == z % 37) ? 1 + z : max_f - (x * 7 + z * 3) % 50; break;  // (every row a site)
          case 6: cls = 1; break;
          default: break;
        }
        if (v > max_f) v = max_f;
        const uint32_t magnitude = v < 0 ? static_cast<uint32_t>(vgt::kInf32) : static_cast<uint32_t>(v);
        in[(static_cast<int64_t>(x) * ny + y) * nz + z] = static_cast<int32_t>(magnitude | (cls ? 0x80000000u : 0u));
      }
  vgt::SdfParams p{};
  p.nx = nx; p.ny = ny; p.nz = nz;
  p.nz_global = nzg;
  p.resolution = 0.37;
  std::vector<unsigned char> scratch(vgt::SweepPassScratchBytes(nx, ny, nzg));
  // the reference, once
  std::vector<float> want(total);
  std::vector<int64_t> f(nx);
  std::vector<uint8_t> neg(nx);
  auto line_of = [&](int y, int z) {
    for (int x = 0; x < nx; x++)
    {
      const int32_t v = in[(static_cast<int64_t>(x) * ny + y) * nz + z];
      neg[x] = v < 0;
      const int64_t a = v & 0x7fffffff;
      f[x] = (a == vgt::kInf32) ? -1 : a;
    }
  };
  float lo = INFINITY, hi = -INFINITY;
  for (int y = 0; y < ny; y++)
    for (int z = 0; z < nz; z++)
    {
      line_of(y, z);
      for (int x = 0; x < nx; x++)
      {
        const int64_t d2 = BruteRow(f, neg, nx, x);
        float w = (d2 == INT64_MAX) ? INFINITY : static_cast<float>(std::sqrt(static_cast<double>(d2)) * p.resolution);
        if (neg[x]) w = -w;
        lo = std::min(lo, w);
        hi = std::max(hi, w);
        want[(static_cast<int64_t>(x) * ny + y) * nz + z] = w;
      }
    }
  for (const int mode : {vgt::kXKernelCoarse, vgt::kXKernelPlain})
  {
    p.x_kernel = mode;
    std::vector<float> out(total, 12345.0f);
    uint32_t minmax[2] = {0xffffffffu, 0u};
    vgt::coarse_dropped.clear();
    reinterpret_cast<int*>(scratch.data())[vgt::kChoiceWord] = 0;
    vgt::LaunchPassXSweepFinalize(in.data(), out.data(), minmax, vgt::SweepScratch{scratch.data(), scratch.size()}, p, nullptr);
    const int ran = reinterpret_cast<int*>(scratch.data())[vgt::kChoiceWord];
    if (ran != (mode == vgt::kXKernelCoarse ? 2 : 1) && failures++ < 10)
      std::printf("KERNEL n %d mode %d: the scratch head says %d\n", n, mode, ran);
    for (int64_t i = 0; i < total; i++)
      if (std::memcmp(&out[i], &want[i], 4) != 0 && failures++ < 10)
        std::printf("MISMATCH n %d mode %d at x %lld y %lld z %lld: got %.9g want %.9g\n", n, mode,
                    static_cast<long long>(i / (ny * nz)), static_cast<long long>(i / nz % ny), static_cast<long long>(i % nz),
                    out[i], want[i]);
    if ((vgt::DecodeOrdered(minmax[0]) != lo || vgt::DecodeOrdered(minmax[1]) != hi) && failures++ < 10)
      std::printf("EXTREMA n %d mode %d\n", n, mode);
    if (mode == vgt::kXKernelPlain)
    {
      if (!vgt::coarse_dropped.empty() && failures++ < 10) std::printf("DROPS n %d: the plain kernel has a chord test\n", n);
      continue;
    }
    // every row the chord test dropped: not on the unfiltered stack when its line ends
    const int zsegs = (nz + 63) / 64;
    std::map<std::pair<int, int>, std::set<int>> stacks;
    uint64_t by_plane[kPlanes] = {};
    for (const vgt::CoarseDrop& d : vgt::coarse_dropped)
    {
      const int y = d.item / zsegs, z0 = (d.item % zsegs) * 64;
      const int z = z0 + std::min(d.lane, nz - 1 - z0);
      auto it = stacks.find({y, z});
      if (it == stacks.end())
      {
        line_of(y, z);
        it = stacks.emplace(std::make_pair(y, z), ReferenceStack(f, nx)).first;
      }
      if (it->second.count(d.row) && failures++ < 10)
        std::printf("DROPPED n %d line (y=%d,z=%d) row %d: on the reference stack when the line ends\n", n, y, z, d.row);
      by_plane[y]++;
      drops_checked++;
    }
    // (the distance-like planes are what the filter is for: it must have removed rows there, or this test checks nothing)
    for (const int y : {0, 5, 7})
      if (by_plane[y] == 0 && failures++ < 10) std::printf("IDLE n %d: the chord test dropped no row of plane %d\n", n, y);
    if ((by_plane[2] != 0 || by_plane[6] != 0) && failures++ < 10)
      std::printf("DROPS n %d: rows dropped on lines with at most two sites\n", n);
  }
}
}  // namespace

int main()
{
  const int lengths[] = {65, 96, 97, 128, 130, 512, 1024};
  for (const int n : lengths) Check(n);
  std::printf("%d lengths, %llu dropped rows checked against the reference stack, %d failures\n",
              static_cast<int>(sizeof(lengths) / sizeof(lengths[0])), static_cast<unsigned long long>(drops_checked), failures);
  return failures ? 1 : 0;
}
