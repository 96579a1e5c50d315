// The per-line routine of the nearest-other-class transform (csrc/nearest_line.hpp) compiled by g++ against the host
// stand-in for the HIP runtime and run on the CPU: the very code the Y and X kernels run, against O(n^2) loops in this
// program.  Built with -fsanitize=address,undefined by tests/test_nearest_line.py (host code only).
//   1. every class pattern of lines of 1 - 10 rows, seeded heights that include "none" and equal heights;
//   2. lines of 64, 65 and 300 rows of the convex case (z - x')^2 and of equal heights, where the stack is as deep as
//      the line allows;
//   3. whole small grids through a plain Z pass, YLine and XLine against a brute-force search over all cells.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "../../voxelized_geometry_tools_amd/csrc/nearest_line.hpp"

namespace
{
long g_mismatches = 0;
int g_deepest = 0;

uint64_t g_state = 0x2545F4914F6CDD1Dull;
uint32_t Next()
{
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return static_cast<uint32_t>(g_state >> 33);
}

// A stack that knows its size: a slot outside it is an error here and under the sanitizer.
struct CheckedStack
{
  std::vector<uint32_t> a, b;
  explicit CheckedStack(int rows) : a(rows > 1 ? rows - 1 : 0), b(rows > 1 ? rows - 1 : 0) {}
  void Put(int slot, uint32_t x, uint32_t y)
  {
    if (slot + 2 > g_deepest) g_deepest = slot + 2;  // (the top entry is in registers)
    a.at(static_cast<size_t>(slot)) = x;
    b.at(static_cast<size_t>(slot)) = y;
  }
  void Get(int slot, uint32_t* x, uint32_t* y) const
  {
    *x = a.at(static_cast<size_t>(slot));
    *y = b.at(static_cast<size_t>(slot));
  }
};

// A line given as arrays: the record of a row is its index.
struct ArrayLine
{
  const std::vector<int>* cls;
  const std::vector<int32_t>* own;  // distance^2 to the row's own nearest other-class cell, -1: none
  std::vector<int>* site;           // out: the row whose site a row takes, -1 none, -2 never written
  uint32_t Load(int r) const { return static_cast<uint32_t>(r); }
  bool IsClass(uint32_t record, int k) const { return (*cls)[record] == k; }
  int32_t Height(uint32_t record, int k) const { return (*cls)[record] != k ? 0 : (*own)[record]; }
  void Emit(int u, int s, uint32_t record, int k) const
  {
    if ((*cls)[static_cast<size_t>(u)] != k || (s >= 0 && record != static_cast<uint32_t>(s))) g_mismatches++;
    if ((*site)[static_cast<size_t>(u)] != -2) g_mismatches++;  // every row is written once
    (*site)[static_cast<size_t>(u)] = s;
  }
};

void CheckLine(const std::vector<int>& cls, const std::vector<int32_t>& own)
{
  const int n = static_cast<int>(cls.size());
  std::vector<int> site(static_cast<size_t>(n), -2);
  const ArrayLine line{&cls, &own, &site};
  CheckedStack stack(n);
  vgt::NearestLine(n, line, stack);
  for (int u = 0; u < n; u++)
  {
    const int k = cls[static_cast<size_t>(u)];
    int64_t best = -1;
    for (int r = 0; r < n; r++)
    {
      const int32_t h = line.Height(static_cast<uint32_t>(r), k);
      if (h < 0) continue;
      const int64_t v = static_cast<int64_t>(u - r) * (u - r) + h;
      if (best < 0 || v < best) best = v;
    }
    const int s = site[static_cast<size_t>(u)];
    bool ok;
    if (best < 0)
      ok = (s == -1);
    else
      ok = s >= 0 && s < n && line.Height(static_cast<uint32_t>(s), k) >= 0 &&
           static_cast<int64_t>(u - s) * (u - s) + line.Height(static_cast<uint32_t>(s), k) == best;
    if (!ok)
    {
      if (g_mismatches < 10) std::printf("line of %d rows: row %d takes %d, best %lld\n", n, u, s, static_cast<long long>(best));
      g_mismatches++;
    }
  }
}

long ShortLines()
{
  long lines = 0;
  for (int n = 1; n <= 10; n++)
    for (uint32_t pattern = 0; pattern < (1u << n); pattern++)
      for (int round = 0; round < 6; round++)
      {
        std::vector<int> cls(static_cast<size_t>(n));
        std::vector<int32_t> own(static_cast<size_t>(n));
        for (int r = 0; r < n; r++)
        {
          cls[static_cast<size_t>(r)] = static_cast<int>((pattern >> r) & 1u);
          const uint32_t v = Next();
          // rounds 0-1: small heights, many equal; 2-3: a third "none"; 4: all none; 5: wide range
          int32_t h = static_cast<int32_t>(v % 5u);
          if (round >= 2 && round <= 3) h = (v % 3u == 0) ? -1 : static_cast<int32_t>((v >> 8) % 20u);
          if (round == 4) h = -1;
          if (round == 5) h = static_cast<int32_t>((v >> 4) % 400u);
          own[static_cast<size_t>(r)] = h;
        }
        CheckLine(cls, own);
        lines++;
      }
  return lines;
}

// The X line (y, z = c) of the diagonal wall filled[x, :, z] = (x == z): row r holds a free cell whose nearest filled
// cell in its own plane is (r, y, r), height (c - r)^2; row c is the filled cell itself.
void ConvexLine(int n, int c)
{
  std::vector<int> cls(static_cast<size_t>(n), 0);
  std::vector<int32_t> own(static_cast<size_t>(n));
  for (int r = 0; r < n; r++) own[static_cast<size_t>(r)] = (c - r) * (c - r);
  if (c >= 0 && c < n)
  {
    cls[static_cast<size_t>(c)] = 1;
    own[static_cast<size_t>(c)] = 1;  // (its nearest free cell is a neighbour)
  }
  CheckLine(cls, own);
}

// Whole grids: a plain Z pass, then the kernels' own lines.
void CheckGrid(int nx, int ny, int nz, uint32_t fill_per_1024)
{
  const size_t n = static_cast<size_t>(nx) * ny * nz;
  std::vector<uint8_t> filled(n);
  for (auto& f : filled) f = (Next() % 1024u) < fill_per_1024;
  std::vector<uint16_t> z_records(n);
  for (int64_t line = 0; line < static_cast<int64_t>(nx) * ny; line++)
    for (int z = 0; z < nz; z++)
    {
      const uint8_t mine = filled[static_cast<size_t>(line * nz + z)];
      int best = -1;
      for (int t = 0; t < nz; t++)  // ascending: the lower z keeps a tie
        if (filled[static_cast<size_t>(line * nz + t)] != mine && (best < 0 || std::abs(t - z) < std::abs(best - z))) best = t;
      z_records[static_cast<size_t>(line * nz + z)] = static_cast<uint16_t>(
          (mine ? vgt::kNearestFilledBit : 0u) | (best < 0 ? vgt::kNearestNoneZ : static_cast<uint32_t>(best)));
    }
  std::vector<uint32_t> y_records(n, 0xffffffffu);
  std::vector<int32_t> nearest(n, -7), d2(n, -7);
  {
    CheckedStack stack(ny);
    for (int x = 0; x < nx; x++)
      for (int z = 0; z < nz; z++)
      {
        const size_t first = static_cast<size_t>(x) * ny * nz + static_cast<size_t>(z);
        const vgt::YLine line{z_records.data() + first, y_records.data() + first, nz, z};
        vgt::NearestLine(ny, line, stack);
      }
  }
  {
    CheckedStack stack(nx);
    const int64_t lines = static_cast<int64_t>(ny) * nz;
    for (int64_t p = 0; p < lines; p++)
    {
      const vgt::XLine line{y_records.data() + p, nearest.data() + p, d2.data() + p, lines, nz,
                            static_cast<int32_t>(p / nz), static_cast<int32_t>(p % nz)};
      vgt::NearestLine(nx, line, stack);
    }
  }
  for (int x = 0; x < nx; x++)
    for (int y = 0; y < ny; y++)
      for (int z = 0; z < nz; z++)
      {
        const size_t c = (static_cast<size_t>(x) * ny + y) * nz + z;
        int64_t best = -1;
        for (int a = 0; a < nx; a++)
          for (int b = 0; b < ny; b++)
            for (int t = 0; t < nz; t++)
              if (filled[(static_cast<size_t>(a) * ny + b) * nz + t] != filled[c])
              {
                const int64_t v = static_cast<int64_t>(a - x) * (a - x) + static_cast<int64_t>(b - y) * (b - y) +
                                  static_cast<int64_t>(t - z) * (t - z);
                if (best < 0 || v < best) best = v;
              }
        bool ok;
        const int32_t got = nearest[c];
        if (best < 0)
          ok = got == -1 && d2[c] == 0x7fffffff;
        else
        {
          ok = got >= 0 && static_cast<size_t>(got) < n && filled[static_cast<size_t>(got)] != filled[c] && d2[c] == best;
          if (ok)
          {
            const int a = got / (ny * nz), b = got / nz % ny, t = got % nz;
            ok = static_cast<int64_t>(a - x) * (a - x) + static_cast<int64_t>(b - y) * (b - y) +
                     static_cast<int64_t>(t - z) * (t - z) == best;
          }
        }
        if (!ok)
        {
          if (g_mismatches < 10)
            std::printf("grid %dx%dx%d cell (%d,%d,%d): nearest %d d2 %d, best %lld\n", nx, ny, nz, x, y, z, got, d2[c],
                        static_cast<long long>(best));
          g_mismatches++;
        }
      }
}
}  // namespace

int main()
{
  const long short_lines = ShortLines();
  std::printf("short lines: %ld\n", short_lines);
  for (int n : {64, 65, 300})
  {
    // the wall's line z = 0: the site nearest to row x is row x / 2, so the lower half of the rows stays on the hull
    g_deepest = 0;
    ConvexLine(n, 0);
    std::printf("convex line of %d rows: hull depth %d\n", n, g_deepest);
    if (2 * g_deepest < n - 1)
    {
      std::printf("the convex line of %d rows kept fewer sites on the hull than its geometry says\n", n);
      g_mismatches++;
    }
    ConvexLine(n, n / 3);
    ConvexLine(n, n + 5);  // (the wall lies outside the line: one class only)
    // equal heights (a filled plane beside the line): every row is its own nearest site, the stack is n deep
    g_deepest = 0;
    CheckLine(std::vector<int>(static_cast<size_t>(n), 0), std::vector<int32_t>(static_cast<size_t>(n), 4));
    std::printf("flat line of %d rows: hull depth %d\n", n, g_deepest);
    if (g_deepest != n)
    {
      std::printf("the flat line of %d rows did not keep every site on the hull\n", n);
      g_mismatches++;
    }
  }
  const int shapes[][3] = {{1, 1, 1}, {3, 2, 5}, {7, 5, 9}, {2, 11, 3}, {12, 6, 14}, {9, 9, 9}};
  for (const auto& s : shapes)
    for (uint32_t fill : {0u, 1u, 30u, 512u, 1000u, 1024u}) CheckGrid(s[0], s[1], s[2], fill);
  std::printf("%ld mismatches\n", g_mismatches);
  std::printf(g_mismatches == 0 ? "PASSED\n" : "FAILED\n");
  return g_mismatches == 0 ? 0 : 1;
}
