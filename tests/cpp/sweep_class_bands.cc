// CPU check of sweep 2's per-band choice between its two copies of the band code (csrc/edt_sweep_kernels.hip: a full band
// of an item with class changes runs the copy without the class-change candidates when two votes say that no lane needs
// them there).  Same set-up as sweep_emulation.cc -- the kernel source compiled by g++ against tests/cpp/hip_shim, one lane
// at a time, against the brute-force contract
//     out(q) = min( min_r (q-r)^2 + |F[r]|,  min over rows r of the other class (q-r)^2 )
// -- on lines BUILT so that bands that may skip the candidates and bands that must keep them lie next to each other, for
// the Y pass (class records) and the X pass (int32 field), at lengths that take 32-bit and 64-bit stack entries.  One
// lane is one line here, so every line decides for itself: stricter than a wave, where one lane's "keep" decides for all.
// The kernel tallies the bands by the copy they ran (class_band_tally); the run fails unless both outcomes are frequent.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <random>
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
constexpr int K = vgt::kBand;
constexpr int kDepth = 40;  // Z extent of the Y-pass volumes: a row's cost is d^2 with d < kDepth

// A line: the class of every row and d, the root of its cost (0: the row is no site).
struct Line
{
  std::vector<uint8_t> cls;
  std::vector<int> d;
  explicit Line(int n) : cls(n, 0), d(n, 0) {}
  int n() const { return static_cast<int>(cls.size()); }
  void other(int row)  // a row of the other class that is no site
  {
    if (row >= 0 && row < n()) cls[row] = 1, d[row] = 0;
  }
};

int failures = 0;
uint64_t tally[2][3];  // [pass: 0 = Y, 1 = X][copy]

void TakeTally(int pass)
{
  for (int i = 0; i < 3; i++)
  {
    tally[pass][i] += vgt::class_band_tally[i];
    vgt::class_band_tally[i] = 0;
  }
}

int64_t BruteRow(const std::vector<int64_t>& f, const std::vector<uint8_t>& neg, int n, int q)
{
  int64_t best = INT64_MAX;
  for (int r = 0; r < n; r++)
  {
    const int64_t dist = static_cast<int64_t>(q - r) * (q - r);
    if (f[r] >= 0) best = std::min(best, dist + f[r]);
    if (neg[r] != neg[q]) best = std::min(best, dist);
  }
  return best;
}

// smallest d >= 1 with d^2 + (K - 1)^2 a square (0: none a volume of kDepth holds), and the root of that square
int ExactRoot(int& delta)
{
  for (int d = 1; d < kDepth; d++)
    for (int e = K; e < 4 * kDepth; e++)
      if (d * d + (K - 1) * (K - 1) == e * e)
      {
        delta = e;
        return d;
      }
  delta = 0;
  return 0;
}

// The lines of length n.
std::vector<Line> BuiltLines(int n)
{
  std::vector<Line> lines;
  const int edge = 3 * K;  // a band's first row, not a word's
  // a single row of the other class whose own cost is 1, no other site: the candidates decide every other row
  for (const int row : {0, 15, 16, 31, 32, n - 1, 70, edge - 1, edge, edge + 1, n - K, n / 2})
  {
    Line l(n);
    l.cls[row] = 1;
    l.d[row] = 1;
    lines.push_back(l);
  }
  // a run of the other class, small costs on every row: the bands far from the run need no candidates
  for (const int first : {n - 20, n / 2, 5, 0})
  {
    Line l(n);
    for (int q = 0; q < n; q++) l.d[q] = 1 + q % 3;
    for (int q = first; q < std::min(n, first + 10); q++) l.cls[q] = 1;
    lines.push_back(l);
  }
  // half-space splits at and around the edges of bands and words, small costs
  for (const int split : {1, 15, 16, 17, 31, 32, 33, n - 1, edge - 1, edge + 1, 2 * 32 - 1, 2 * 32 + 1})
  {
    Line l(n);
    for (int q = 0; q < n; q++)
    {
      l.cls[q] = q >= split;
      l.d[q] = 1 + q % 2;
    }
    lines.push_back(l);
  }
  // B = delta^2 exactly (may skip) and B = delta^2 + 1 (must keep): ONE site, so the top entry is known; the other class
  // delta rows above the band's top row or delta rows below its first row; the site at the band's far end, where B is
  // taken at the row whose candidate is the nearest (the candidate wins by one when B = delta^2 + 1), and at its near end.
  int exact_delta = 0;
  const int exact_d = ExactRoot(exact_delta);
  for (const int r0 : {edge, 2 * 32, 4 * 32 - K, n / K * K - 2 * K})
    for (const bool plus_one : {false, true})
    {
      const int d = plus_one ? 1 : exact_d, delta = plus_one ? K - 1 : exact_delta;
      if (d == 0 || r0 - delta < 0 || r0 + K - 1 + delta >= n) continue;
      for (const bool above : {false, true})
        for (const bool site_far : {false, true})
        {
          Line l(n);
          const int near_row = above ? r0 + K - 1 : r0, far_row = above ? r0 : r0 + K - 1;
          l.d[site_far ? far_row : near_row] = d;
          for (int j = 0; j < 3; j++) l.other(above ? near_row + delta + j : near_row - delta - j);
          lines.push_back(l);
        }
    }
  // lines without any site: one class, and with a class change (every result is a candidate's)
  lines.emplace_back(n);
  {
    Line l(n);
    for (int q = 40; q < n; q++) l.cls[q] = 1;
    lines.push_back(l);
  }
  return lines;
}

// Random lines with few class changes and distance-like costs (roots below kDepth).
std::vector<Line> RandomLines(int n, int count, std::mt19937& rng)
{
  std::vector<Line> lines;
  for (int i = 0; i < count; i++)
  {
    Line l(n);
    const int p_flip = 1 + static_cast<int>(rng() % 3), p_site = 30 + static_cast<int>(rng() % 71);
    const int mode = static_cast<int>(rng() % 3);
    int cls = rng() & 1;
    const int centre = static_cast<int>(rng() % n);
    for (int q = 0; q < n; q++)
    {
      if (static_cast<int>(rng() % 1000) < 3 * p_flip) cls ^= 1;
      l.cls[q] = static_cast<uint8_t>(cls);
      int d = 0;
      switch (mode)
      {
        case 0: d = 1 + static_cast<int>(rng() % 3); break;
        case 1: d = 1 + static_cast<int>(rng() % (kDepth - 1)); break;
        default: d = 1 + std::min(kDepth - 2, std::abs(q - centre) / 8); break;
      }
      l.d[q] = (static_cast<int>(rng() % 100) < p_site) ? d : 0;
    }
    lines.push_back(l);
  }
  return lines;
}

// Class records of a class volume, by the definition (as in sweep_emulation.cc).
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

// Y pass: line i is the Y line (x = i, z = 0) of a volume whose Z lines realise the costs: row y of class c with root d is
// c along all of Z but for the voxel at z = d.  (The other Z positions are lines of their own and are checked as well.)
void CheckY(const std::vector<Line>& lines)
{
  const int nx = static_cast<int>(lines.size()), ny = lines[0].n(), nz = kDepth;
  const int64_t total = static_cast<int64_t>(nx) * ny * nz;
  std::vector<uint8_t> cls(total);
  for (int x = 0; x < nx; x++)
    for (int y = 0; y < ny; y++)
      for (int z = 0; z < nz; z++)
        cls[(static_cast<size_t>(x) * ny + y) * nz + z] = lines[x].cls[y] ^ static_cast<uint8_t>(z != 0 && z == lines[x].d[y]);
  const std::vector<vgt::ClassRecord> rec = RecordsOf(cls, nx, ny, nz);
  std::vector<int32_t> out(total, 12345);
  vgt::SdfParams p{};
  p.nx = nx; p.ny = ny; p.nz = nz;
  p.resolution = 0.01;
  std::vector<unsigned char> scratch(vgt::SweepPassScratchBytes(nx, ny, nz));
  vgt::LaunchPassYSweepRecords(rec.data(), out.data(), vgt::SweepScratch{scratch.data(), scratch.size()}, p, nullptr);
  TakeTally(0);
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
          std::printf("Y MISMATCH n %d line %d z %d row %d: got %d want %lld\n", ny, x, z, y, got,
                      static_cast<long long>(signed_want));
      }
    }
}

// X pass: line i is the X line (y = 0, z = i) of the int32 field, costs d^2 (+ `bump` on every site: costs that are no squares).
void CheckX(const std::vector<Line>& lines, bool border, int bump)
{
  const int nx = lines[0].n(), ny = 1, nz = static_cast<int>(lines.size());
  const int64_t total = static_cast<int64_t>(nx) * nz;
  std::vector<int32_t> in(total);
  std::vector<int64_t> want_d2(total);
  std::vector<int64_t> f(nx);
  for (int z = 0; z < nz; z++)
  {
    const Line& l = lines[z];
    for (int x = 0; x < nx; x++)
    {
      f[x] = l.d[x] ? static_cast<int64_t>(l.d[x]) * l.d[x] + bump : -1;
      const uint32_t v = f[x] < 0 ? static_cast<uint32_t>(vgt::kInf32) : static_cast<uint32_t>(f[x]);
      in[static_cast<int64_t>(x) * nz + z] = static_cast<int32_t>(v | (l.cls[x] ? 0x80000000u : 0u));
    }
    for (int x = 0; x < nx; x++)
    {
      int64_t d2 = BruteRow(f, l.cls, nx, x);
      if (border)
      {
        int64_t b = std::min(x + 1, nx - x);
        if (nz > 1) b = std::min<int64_t>(b, std::min(z + 1, nz - z));
        d2 = std::min(d2, b * b);
      }
      want_d2[static_cast<int64_t>(x) * nz + z] = d2;
    }
  }
  std::vector<unsigned char> scratch(vgt::SweepPassScratchBytes(nx, ny, nz));
  std::vector<float> out(total, 12345.0f);
  const double resolution = 0.37;
  vgt::SdfParams p{};
  p.nx = nx; p.ny = ny; p.nz = nz;
  p.resolution = resolution;
  p.add_virtual_border = border ? 1 : 0;
  uint32_t minmax[2] = {0xffffffffu, 0u};
  vgt::LaunchPassXSweepFinalize(in.data(), out.data(), minmax, vgt::SweepScratch{scratch.data(), scratch.size()}, p, nullptr);
  TakeTally(1);
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t i = 0; i < total; i++)
  {
    const int64_t d2 = want_d2[i];
    float want = (d2 == INT64_MAX) ? INFINITY : static_cast<float>(std::sqrt(static_cast<double>(d2)) * resolution);
    if (in[i] < 0) want = -want;
    lo = std::min(lo, want);
    hi = std::max(hi, want);
    const float got = out[i];
    if (std::memcmp(&got, &want, 4) != 0 && failures++ < 10)
      std::printf("X MISMATCH n %d border %d bump %d line %d row %d d2 %lld: got %.9g want %.9g\n", nx, border, bump,
                  static_cast<int>(i % nz), static_cast<int>(i / nz), static_cast<long long>(d2), got, want);
  }
  const float got_lo = vgt::DecodeOrdered(minmax[0]), got_hi = vgt::DecodeOrdered(minmax[1]);
  if ((got_lo != lo || got_hi != hi) && failures++ < 10)
    std::printf("X EXTREMA n %d border %d: got (%g, %g) want (%g, %g)\n", nx, border, got_lo, got_hi, lo, hi);
}
}  // namespace

int main()
{
  std::mt19937 rng(777);
  int line_count = 0;
  // 150: a partial band and a partial word; 1024: the longest line of 32-bit entries; 1040: 64-bit entries
  for (const int n : {150, 1024, 1040})
  {
    std::vector<Line> lines = BuiltLines(n);
    const std::vector<Line> random = RandomLines(n, n == 150 ? 40 : 12, rng);
    lines.insert(lines.end(), random.begin(), random.end());
    line_count += static_cast<int>(lines.size());
    CheckY(lines);
    CheckX(lines, false, 0);  // (small costs: the table copies of the band code where the entries are 32 bits wide)
    CheckX(lines, true, 0);
    CheckX(lines, false, 600);  // (costs above the table's range)
  }
  const char* names[2] = {"Y", "X"};
  for (int pass = 0; pass < 2; pass++)
    std::printf("%s pass: %llu bands with candidates after the second vote, %llu without candidates, %llu with candidates after the first vote\n",
                names[pass], static_cast<unsigned long long>(tally[pass][0]), static_cast<unsigned long long>(tally[pass][1]),
                static_cast<unsigned long long>(tally[pass][2]));
  const uint64_t skipped = tally[0][1] + tally[1][1];
  const uint64_t kept = tally[0][0] + tally[0][2] + tally[1][0] + tally[1][2];
  std::printf("%d lines per pass, %d mismatches, %llu bands skipped, %llu bands kept (band %d)\n", line_count, failures,
              static_cast<unsigned long long>(skipped), static_cast<unsigned long long>(kept), K);
  if (failures) return 1;
  for (int pass = 0; pass < 2; pass++)
    if (tally[pass][1] < 1000 || tally[pass][0] + tally[pass][2] < 1000)
    {
      std::printf("too few bands of one outcome in the %s pass\n", names[pass]);
      return 2;
    }
  return 0;
}
