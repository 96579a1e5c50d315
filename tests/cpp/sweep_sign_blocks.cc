// CPU check of sweep 2's sign words (csrc/edt_sweep_kernels.hip compiled by g++ against tests/cpp/hip_shim, lanes one at a
// time, like sweep_emulation.cc): sweep 2 takes the words sweep 1 wrote in blocks of several words, a block ahead.  Lines
// whose lengths straddle words and blocks, with class changes where the block bookkeeping could slip -- none, one at the
// first or the last row of a word, at the block seams, at every row -- and items that take the fill path (no site and no
// change in any lane) or hold a lane without any site among lanes that have some, run through both passes against the
// brute-force line transform.  Under VGT_HOST_EMULATION every lane poisons its words of the scratch slot when it takes an
// item (three slots here, so slots are used again and again) and the kernel asserts at every use of a sign word that it is
// not poison: sweep 2 never reads a word that sweep 1 has not written for this item.  This file is built with assertions
// on and counts the uses, so that the assertion is known to have stood on the paths it guards.
#ifdef NDEBUG
#error "the kernel's assertions are the check: build without NDEBUG"
#endif
#include <hip/hip_runtime.h>

#include <cstdio>
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
constexpr int kWordRows = 32;

// Class patterns of lines of n rows: one class (either), a change at every row, and one change in front of row s for every
// s that is the first or the last row of a word -- of every word, so every seam between two blocks is among them whatever
// the block size and the end it is counted from (the kernel counts from the line's last word) -- and in front of rows 127,
// 128, 255, 256 and the last row.
std::vector<std::vector<uint8_t>> Patterns(int n)
{
  std::vector<std::vector<uint8_t>> out;
  out.emplace_back(n, uint8_t{0});
  out.emplace_back(n, uint8_t{1});
  std::vector<uint8_t> every(n);
  for (int r = 0; r < n; r++) every[r] = static_cast<uint8_t>(r & 1);
  out.push_back(every);
  const int nwords = (n + kWordRows - 1) / kWordRows;
  std::set<int> seams = {127, 128, 255, 256, n - 1};
  for (int w = 0; w < nwords; w++)
  {
    seams.insert(w * kWordRows);
    seams.insert(w * kWordRows + kWordRows - 1);
  }
  for (const int s : seams)
  {
    if (s <= 0 || s >= n) continue;
    std::vector<uint8_t> line(n);
    for (int r = 0; r < n; r++) line[r] = static_cast<uint8_t>(r >= s);
    out.push_back(line);
  }
  return out;
}

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

// X pass: lines along x.  Items are (y, 64 lanes of z).  y = 0, 4: the patterns, every lane with sites; y = 1, 2: no site and
// no change in any lane (the fill path), one class each; y = 3: the patterns, every seventh lane without any site.
void CheckX(int n, bool border)
{
  const std::vector<std::vector<uint8_t>> patterns = Patterns(n);
  const int nx = n, ny = 5, nz = static_cast<int>(patterns.size());
  const int64_t total = static_cast<int64_t>(nx) * ny * nz;
  const int64_t max_f = static_cast<int64_t>(nz - 1) * (nz - 1) + static_cast<int64_t>(ny - 1) * (ny - 1);
  std::vector<int32_t> in(total);
  for (int y = 0; y < ny; y++)
    for (int z = 0; z < nz; z++)
      for (int x = 0; x < nx; x++)
      {
        int64_t v = vgt::kInf32;
        uint8_t cls = patterns[z][x];
        if (y == 1 || y == 2)
          cls = static_cast<uint8_t>(y - 1);
        else if (!(y == 3 && z % 7 == 3) && (x + z) % 3 != 0)
          v = 1 + (static_cast<int64_t>(x) * 7 + z * 13 + y) % 97 * 5 % std::max<int64_t>(1, std::min<int64_t>(max_f, 400));
        in[(static_cast<int64_t>(x) * ny + y) * nz + z] = static_cast<int32_t>(static_cast<uint32_t>(v) | (cls ? 0x80000000u : 0u));
      }
  std::vector<unsigned char> scratch(vgt::SweepPassScratchBytes(nx, ny, nz));
  std::vector<float> out(total, 12345.0f);
  vgt::SdfParams p{};
  p.nx = nx; p.ny = ny; p.nz = nz;
  p.resolution = 0.37;
  p.add_virtual_border = border ? 1 : 0;
  uint32_t minmax[2] = {0xffffffffu, 0u};
  const uint64_t reads_before = vgt::sign_word_reads;
  vgt::LaunchPassXSweepFinalize(in.data(), out.data(), minmax, vgt::SweepScratch{scratch.data(), scratch.size()}, p, nullptr);
  const uint64_t reads = vgt::sign_word_reads - reads_before;
  std::vector<int64_t> f(nx);
  std::vector<uint8_t> neg(nx);
  float lo = INFINITY, hi = -INFINITY;
  for (int y = 0; y < ny; y++)
    for (int z = 0; z < nz; z++)
    {
      for (int x = 0; x < nx; x++)
      {
        const int32_t v = in[(static_cast<int64_t>(x) * ny + y) * nz + z];
        neg[x] = v < 0;
        const int64_t a = v & 0x7fffffff;
        f[x] = (a == vgt::kInf32) ? -1 : a;
      }
      for (int x = 0; x < nx; x++)
      {
        int64_t d2 = BruteRow(f, neg, nx, x);
        if (border)
        {
          int64_t b = INT64_MAX;
          if (nx > 1) b = std::min<int64_t>(b, std::min(x + 1, nx - x));
          if (ny > 1) b = std::min<int64_t>(b, std::min(y + 1, ny - y));
          if (nz > 1) b = std::min<int64_t>(b, std::min(z + 1, nz - z));
          if (b != INT64_MAX) d2 = std::min(d2, b * b);
        }
        float want = (d2 == INT64_MAX) ? INFINITY : static_cast<float>(std::sqrt(static_cast<double>(d2)) * p.resolution);
        if (neg[x]) want = -want;
        lo = std::min(lo, want);
        hi = std::max(hi, want);
        const float got = out[(static_cast<int64_t>(x) * ny + y) * nz + z];
        if (std::memcmp(&got, &want, 4) != 0 && failures++ < 10)
          std::printf("X MISMATCH n %d border %d line (y=%d,z=%d) row %d: got %.9g want %.9g\n", n, border, y, z, x, got, want);
      }
    }
  if ((vgt::DecodeOrdered(minmax[0]) != lo || vgt::DecodeOrdered(minmax[1]) != hi) && failures++ < 10)
    std::printf("X EXTREMA n %d border %d\n", n, border);
  // every lane of every item uses every word of its line once (and the word below it a second time, for its top bit)
  const uint64_t least = static_cast<uint64_t>(ny) * ((nz + 63) / 64) * 64 * ((n + kWordRows - 1) / kWordRows);
  if (reads < least && failures++ < 10)
    std::printf("X READS n %d: %llu uses of a sign word, at least %llu expected\n", n, static_cast<unsigned long long>(reads),
                static_cast<unsigned long long>(least));
}

// Class records of a class volume, by the definition (csrc/vgt_internal.hpp), as in sweep_emulation.cc.
std::vector<vgt::ClassRecord> RecordsOf(const std::vector<uint8_t>& cls, int nx, int ny, int nz)
{
  const int nwords = static_cast<int>(vgt::RecordWords(nz));
  std::vector<vgt::ClassRecord> rec(static_cast<size_t>(nx) * nwords * ny + vgt::kRecordPadding);
  for (auto& r : rec) r = vgt::ClassRecord{0xdeadbeefu, 0xdeadbeefu, 12345u, 54321u};  // (padding: never used)
  for (int x = 0; x < nx; x++)
    for (int y = 0; y < ny; y++)
    {
      const uint8_t* line = &cls[(static_cast<size_t>(x) * ny + y) * nz];
      bool any = false;
      for (int z = 0; z + 1 < nz; z++) any = any || line[z] != line[z + 1];
      for (int w = 0; w < nwords; w++)
      {
        vgt::ClassRecord r{0, 0, vgt::kRecordNoneBelow, vgt::kRecordNoneAbove};
        for (int k = 0; k < 64; k++)
        {
          const int z = std::min(64 * w + k, nz - 1);
          if (line[z]) (k < 32 ? r.mask_lo : r.mask_hi) |= 1u << (k & 31);
        }
        for (int t = 64 * w - 1; t >= 0; t--)
          if (line[t] != line[t + 1])
          {
            r.below2 = static_cast<uint32_t>(2 * (t - 64 * w)) + vgt::kRecordBias;
            break;
          }
        for (int t = 64 * w + 63; t + 1 < nz; t++)
          if (line[t] != line[t + 1])
          {
            r.above2 = static_cast<uint32_t>(2 * (t - 64 * w)) + vgt::kRecordBias;
            break;
          }
        if (!any) r.above2 = vgt::kRecordNoSite;
        rec[(static_cast<size_t>(x) * nwords + w) * ny + y] = r;
      }
    }
  return rec;
}

// Y pass: lines along y, lanes along z, items are (x, 64 lanes of z).  x = 0, 4: the patterns (a row has sites wherever its
// lanes differ); x = 1, 2: one class (the fill path); x = 3: every lane runs through the same pattern -- no row has a site,
// the class changes along the lines alone decide (a lane without any site is, in this pass, a whole item without any).
void CheckY(int n)
{
  const std::vector<std::vector<uint8_t>> patterns = Patterns(n);
  const int nx = 5, ny = n, nz = static_cast<int>(patterns.size());
  const int64_t total = static_cast<int64_t>(nx) * ny * nz;
  std::vector<uint8_t> cls(total);
  for (int x = 0; x < nx; x++)
    for (int y = 0; y < ny; y++)
      for (int z = 0; z < nz; z++)
      {
        uint8_t c = patterns[z][y];
        if (x == 1 || x == 2) c = static_cast<uint8_t>(x - 1);
        if (x == 3) c = patterns[patterns.size() / 2][y];
        cls[(static_cast<size_t>(x) * ny + y) * nz + z] = c;
      }
  const std::vector<vgt::ClassRecord> rec = RecordsOf(cls, nx, ny, nz);
  std::vector<int32_t> out(total, 12345);
  vgt::SdfParams p{};
  p.nx = nx; p.ny = ny; p.nz = nz;
  p.resolution = 0.01;
  std::vector<unsigned char> scratch(vgt::SweepPassScratchBytes(nx, ny, nz));
  const uint64_t reads_before = vgt::sign_word_reads;
  vgt::LaunchPassYSweepRecords(rec.data(), out.data(), vgt::SweepScratch{scratch.data(), scratch.size()}, p, nullptr);
  const uint64_t reads = vgt::sign_word_reads - reads_before;
  std::vector<int64_t> f(ny);
  std::vector<uint8_t> neg(ny);
  for (int x = 0; x < nx; x++)
    for (int z = 0; z < nz; z++)
    {
      for (int y = 0; y < ny; y++)
      {
        const uint8_t* line = &cls[(static_cast<size_t>(x) * ny + y) * nz];
        neg[y] = line[z];
        int64_t d = -1;
        for (int k = 1; k < nz; k++)
          if ((z - k >= 0 && line[z - k] != line[z]) || (z + k < nz && line[z + k] != line[z]))
          {
            d = k;
            break;
          }
        f[y] = d < 0 ? -1 : d * d;
      }
      for (int y = 0; y < ny; y++)
      {
        int64_t want = BruteRow(f, neg, ny, y);
        want = (want == INT64_MAX) ? vgt::kInf32 : want;
        const int64_t signed_want = neg[y] ? -want : want;
        const int32_t raw = out[(static_cast<int64_t>(x) * ny + y) * nz + z];
        const int32_t got = (raw < 0) ? -(raw & 0x7fffffff) : raw;
        if (got != signed_want && failures++ < 10)
          std::printf("Y MISMATCH n %d line (x=%d,z=%d) row %d: got %d want %lld\n", n, x, z, y, got,
                      static_cast<long long>(signed_want));
      }
    }
  const uint64_t least = static_cast<uint64_t>(nx) * ((nz + 63) / 64) * 64 * ((n + kWordRows - 1) / kWordRows);
  if (reads < least && failures++ < 10)
    std::printf("Y READS n %d: %llu uses of a sign word, at least %llu expected\n", n, static_cast<unsigned long long>(reads),
                static_cast<unsigned long long>(least));
}
}  // namespace

int main()
{
  // (1056 rows: 64-bit entries)
  const int lengths[] = {1, 31, 32, 33, 96, 127, 128, 129, 160, 255, 256, 257, 383, 1024, 1056};
  for (const int n : lengths)
  {
    CheckX(n, false);
    if (n == 33 || n == 257) CheckX(n, true);  // (the virtual border keeps all-empty items off the fill path)
    CheckY(n);
  }
  std::printf("blocks of %d words; %d lengths, %llu uses of a sign word checked, %d failures\n", vgt::kInfoBlock, static_cast<int>(sizeof(lengths) / sizeof(lengths[0])),
              static_cast<unsigned long long>(vgt::sign_word_reads), failures);
  return failures ? 1 : 0;
}
