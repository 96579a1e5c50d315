// CPU check of sweep 1's ring checks (csrc/edt_sweep_kernels.hip compiled by g++ against tests/cpp/hip_shim, lanes one at a
// time, like sweep_emulation.cc): on lines that spill at every check -- the scenes of tests/test_gpu_sweep_ring_checks.py,
// as the X pass meets them -- a check spills ONE chunk or none.  The kernel asserts that itself under VGT_HOST_EMULATION
// (this file is built with assertions on); here the spills are counted against what the lines must cause, so that the
// assertion is known to have been reached on the path it guards, and the results are compared with a brute-force line
// transform.
#ifdef NDEBUG
#error "the kernel's assertions are the check: build without NDEBUG"
#endif
#include <hip/hip_runtime.h>

#include <cstdio>
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

// scene 0: staircase (every row a hull point), 1: the staircase interrupted by rows without a site and knocked down by
// rows with small distances, 2 / 3: salt-like lines (5 % / 50 % of the rows are sites of random height)
void Check(int nx, int ny, int nz, int scene)
{
  const int64_t total = static_cast<int64_t>(nx) * ny * nz;
  std::vector<int32_t> in(total);
  uint32_t state = 12345u + static_cast<uint32_t>(scene);
  auto rnd = [&]() { return state = state * 1664525u + 1013904223u, state >> 8; };
  for (int x = 0; x < nx; x++)
    for (int y = 0; y < ny; y++)
      for (int z = 0; z < nz; z++)
      {
        const int64_t far = static_cast<int64_t>(nz - 1 - z) * (nz - 1 - z) + 1;
        int64_t v = far;
        if (scene == 1) v = (x % 48 < 30) ? far : (x % 48 == 47 ? 1 + (z & 1) : vgt::kInf32);
        if (scene >= 2) v = (static_cast<int>(rnd() % 100) < (scene == 2 ? 5 : 50)) ? 1 + rnd() % 50 : vgt::kInf32;
        in[(static_cast<int64_t>(x) * ny + y) * nz + z] = static_cast<int32_t>(v);
      }
  std::vector<unsigned char> scratch(vgt::SweepPassScratchBytes(nx, ny, nz));
  std::vector<float> out(total, 12345.0f);
  vgt::SdfParams p{};
  p.nx = nx; p.ny = ny; p.nz = nz;
  p.resolution = 0.25;
  uint32_t minmax[2] = {0xffffffffu, 0u};
  const uint64_t checks_before = vgt::ring_checks, spills_before = vgt::ring_spills;
  vgt::LaunchPassXSweepFinalize(in.data(), out.data(), minmax, vgt::SweepScratch{scratch.data(), scratch.size()}, p, nullptr);
  const uint64_t checks = vgt::ring_checks - checks_before, spills = vgt::ring_spills - spills_before;
  for (int y = 0; y < ny; y++)
    for (int z = 0; z < nz; z++)
      for (int x = 0; x < nx; x++)
      {
        int64_t best = INT64_MAX;
        for (int r = 0; r < nx; r++)
        {
          const int64_t f = in[(static_cast<int64_t>(r) * ny + y) * nz + z];
          if (f != vgt::kInf32) best = std::min(best, static_cast<int64_t>(x - r) * (x - r) + f);
        }
        const float want = best == INT64_MAX ? INFINITY : static_cast<float>(std::sqrt(static_cast<double>(best)) * p.resolution);
        const float got = out[(static_cast<int64_t>(x) * ny + y) * nz + z];
        if (std::memcmp(&got, &want, 4) != 0 && failures++ < 10)
          std::printf("MISMATCH %dx%dx%d scene %d line (y=%d,z=%d) row %d: got %.9g want %.9g\n", nx, ny, nz, scene, y, z, x, got, want);
      }
  // The staircase pushes every row and pops none: whatever does not fit the ring has been spilled, a chunk at a time.
  const bool packed = vgt::PackedEntries(nx, static_cast<int64_t>(nz - 1) * (nz - 1) + static_cast<int64_t>(ny - 1) * (ny - 1));
  const int ring = packed ? vgt::RingShape<true>::kRing : vgt::RingShape<false>::kRing;
  const int chunk = packed ? vgt::RingShape<true>::kChunk : vgt::RingShape<false>::kChunk;
  const uint64_t lanes = static_cast<uint64_t>(ny) * ((nz + 63) / 64) * 64;  // (lanes past the grid repeat its last line)
  if (scene == 0 && nx + 4 > ring)
  {
    const uint64_t least = lanes * static_cast<uint64_t>((nx + 4 - ring) / chunk);
    if (spills < least && failures++ < 10)
      std::printf("SPILLS %dx%dx%d: %llu spills, the staircase needs at least %llu\n", nx, ny, nz,
                  static_cast<unsigned long long>(spills), static_cast<unsigned long long>(least));
  }
  if (spills > checks && failures++ < 10) std::printf("SPILLS %dx%dx%d scene %d: more spills than checks\n", nx, ny, nz, scene);
  std::printf("%dx%dx%d scene %d (%s entries): %llu checks, %llu spills\n", nx, ny, nz, scene, packed ? "32-bit" : "64-bit",
              static_cast<unsigned long long>(checks), static_cast<unsigned long long>(spills));
}
}  // namespace

int main()
{
  const int shapes[][3] = {{33, 2, 64}, {65, 2, 70}, {200, 2, 1}, {1024, 1, 65}, {1100, 1, 65}};
  for (const auto& s : shapes)
    for (int scene = 0; scene < 4; scene++) Check(s[0], s[1], s[2], scene);
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
