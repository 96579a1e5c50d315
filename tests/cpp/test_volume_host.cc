// RasterizeSphereModel, RasterizeSphereModelIntoOccupancyMap and FindPointsOnSphereModel of the C++ host layer
// (include/vgt_hip/body_volumes.hpp) against an in-file restatement of vgt_hip_rasterize_spheres and
// vgt_hip_spheres_cover_points (include/vgt_hip.h), bit for bit.
//   test_volume_host              the restatement against hand-derived answers, the argument errors, and the layer on
//                                 device 0 against the restatement
//   test_volume_host --no-device  the first two only: nothing here touches a device
#include <vgt_hip.h>
#include <vgt_hip/body_volumes.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <vector>

using namespace vgt_hip;

static int g_failures = 0;
#define CHECK(cond)                                                    \
  do                                                                   \
  {                                                                    \
    if (!(cond))                                                       \
    {                                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      g_failures++;                                                    \
    }                                                                  \
  } while (0)

template <typename Fn>
static bool ThrowsInvalidArgument(const Fn& fn, const char* needle = nullptr)
{
  try
  {
    fn();
  }
  catch (const std::invalid_argument& e)
  {
    return needle == nullptr || std::strstr(e.what(), needle) != nullptr;
  }
  catch (...)
  {
  }
  return false;
}

// ---- the restatement: brute force, every cell or point against every sphere, in the order include/vgt_hip.h gives ----
namespace restated
{
struct Sphere
{
  double c[3], R;
  bool usable;
};

// the world centre and R of sphere s in configuration b; with M (grid_from_world, or nullptr) the centre in the grid frame
static Sphere Place(const SphereModel& model, const std::vector<double>& poses, int64_t num_links, size_t b, size_t s,
                    double padding, const double* M)
{
  Sphere out{{0.0, 0.0, 0.0}, 0.0, false};
  const int32_t link = model.link[s];
  if (link < 0 || link >= num_links) return out;
  const double* m = poses.data() + (b * static_cast<size_t>(num_links) + static_cast<size_t>(link)) * 16;
  const double x = model.xyzr[s][0], y = model.xyzr[s][1], z = model.xyzr[s][2];
  double w[3];
  for (int r = 0; r < 3; r++) w[r] = ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r];
  out.R = model.xyzr[s][3] + padding;
  out.usable = std::isfinite(w[0]) && std::isfinite(w[1]) && std::isfinite(w[2]) && std::isfinite(out.R) && out.R >= 0.0;
  for (int a = 0; a < 3; a++) out.c[a] = M ? M[a] * w[0] + M[4 + a] * w[1] + M[8 + a] * w[2] + M[12 + a] : w[a];
  out.usable = out.usable && std::isfinite(out.c[0]) && std::isfinite(out.c[1]) && std::isfinite(out.c[2]);
  return out;
}

static bool Covers(const Sphere& sphere, const double q[3])
{
  const double dx = q[0] - sphere.c[0], dy = q[1] - sphere.c[1], dz = q[2] - sphere.c[2];
  return sphere.usable && ((dx * dx + dy * dy) + dz * dz) <= sphere.R * sphere.R;
}

static std::vector<int32_t> Rasterize(int64_t nx, int64_t ny, int64_t nz, double resolution, const double* M,
                                      const SphereModel& model, const std::vector<double>& poses, int64_t num_links,
                                      double padding, int64_t base, const std::vector<int32_t>* keep = nullptr)
{
  std::vector<int32_t> first = keep ? *keep : std::vector<int32_t>(static_cast<size_t>(nx * ny * nz), -1);
  const size_t b_count = num_links > 0 ? poses.size() / (static_cast<size_t>(num_links) * 16) : 0;
  for (size_t b = 0; b < b_count; b++)
    for (size_t s = 0; s < model.link.size(); s++)
    {
      const Sphere sphere = Place(model, poses, num_links, b, s, padding, M);
      for (int64_t x = 0; x < nx; x++)
        for (int64_t y = 0; y < ny; y++)
          for (int64_t z = 0; z < nz; z++)
          {
            const double q[3] = {(static_cast<double>(x) + 0.5) * resolution, (static_cast<double>(y) + 0.5) * resolution,
                                 (static_cast<double>(z) + 0.5) * resolution};
            int32_t& entry = first[static_cast<size_t>((x * ny + y) * nz + z)];
            const uint32_t key = static_cast<uint32_t>(base + static_cast<int64_t>(b));
            if (Covers(sphere, q) && key < static_cast<uint32_t>(entry)) entry = static_cast<int32_t>(key);
          }
    }
  return first;
}

static PointsOnSphereModel Cover(const std::vector<float>& points, const double* T, const SphereModel& model,
                                 const std::vector<double>& poses, int64_t num_links, double padding)
{
  PointsOnSphereModel out;
  const size_t n = points.size() / 3;
  const size_t b_count = num_links > 0 ? poses.size() / (static_cast<size_t>(num_links) * 16) : 0;
  out.filtered = points;
  for (size_t i = 0; i < n; i++)
  {
    const double p[3] = {static_cast<double>(points[3 * i]), static_cast<double>(points[3 * i + 1]),
                         static_cast<double>(points[3 * i + 2])};
    double q[3];
    for (int r = 0; r < 3; r++) q[r] = T ? ((T[r] * p[0] + T[4 + r] * p[1]) + T[8 + r] * p[2]) + T[12 + r] : p[r];
    bool ok = true;
    for (int r = 0; r < 3; r++) ok = ok && std::isfinite(p[r]) && std::isfinite(q[r]);
    int32_t found_b = -1, found_s = -1;
    for (size_t b = 0; ok && b < b_count && found_b < 0; b++)
      for (size_t s = 0; s < model.link.size() && found_b < 0; s++)
        if (Covers(Place(model, poses, num_links, b, s, padding, nullptr), q))
        {
          found_b = static_cast<int32_t>(b);
          found_s = static_cast<int32_t>(s);
        }
    out.first_configuration.push_back(found_b);
    out.first_sphere.push_back(found_s);
    if (found_b >= 0)
      for (int a = 0; a < 3; a++) out.filtered[3 * i + static_cast<size_t>(a)] = std::numeric_limits<float>::quiet_NaN();
  }
  return out;
}
}  // namespace restated

static std::vector<double> Pose(double x, double y, double z)
{
  const Isometry3 t = Isometry3::Translation(x, y, z);
  return std::vector<double>(t.m.begin(), t.m.end());
}

static void Append(std::vector<double>& poses, const std::vector<double>& pose)
{
  poses.insert(poses.end(), pose.begin(), pose.end());
}

static SphereModel OneSphere(double radius)
{
  SphereModel model;
  model.link = {0};
  model.xyzr = {{{0.0, 0.0, 0.0, radius}}};
  return model;
}

static int64_t Count(const std::vector<int32_t>& first)
{
  int64_t covered = 0;
  for (int32_t v : first) covered += v >= 0;
  return covered;
}

template <typename T>
static bool SameBytes(const std::vector<T>& a, const std::vector<T>& b)
{
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// floats: the same bits, or NaN in both
static bool SameFloats(const std::vector<float>& a, const std::vector<float>& b)
{
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (!(std::isnan(a[i]) && std::isnan(b[i])) && std::memcmp(&a[i], &b[i], sizeof(float)) != 0) return false;
  return true;
}

static int RunNoDevice()
{
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  // 8 x 9 x 10 at resolution 0.25; the centre of cell (3, 4, 5) is (0.875, 1.125, 1.375), exactly
  const int64_t nx = 8, ny = 9, nz = 10;
  const double res = 0.25;
  const std::vector<double> centre = Pose(0.875, 1.125, 1.375);
  auto at = [&](const std::vector<int32_t>& first, int64_t x, int64_t y, int64_t z) {
    return first[static_cast<size_t>((x * ny + y) * nz + z)];
  };
  // the restatement against answers derived by hand
  {
    std::vector<int32_t> first = restated::Rasterize(nx, ny, nz, res, nullptr, OneSphere(0.0), centre, 1, 0.0, 0);
    CHECK(Count(first) == 1 && at(first, 3, 4, 5) == 0);  // R == 0 covers the location that equals the centre
    first = restated::Rasterize(nx, ny, nz, res, nullptr, OneSphere(0.25), centre, 1, 0.0, 0);
    CHECK(Count(first) == 7 && at(first, 3, 4, 5) == 0);  // d^2 == R^2 == 0.0625: the six face neighbours
    CHECK(at(first, 2, 4, 5) == 0 && at(first, 4, 4, 5) == 0 && at(first, 3, 3, 5) == 0 && at(first, 3, 5, 5) == 0 &&
          at(first, 3, 4, 4) == 0 && at(first, 3, 4, 6) == 0);
    first = restated::Rasterize(nx, ny, nz, res, nullptr, OneSphere(std::nextafter(0.25, 0.0)), centre, 1, 0.0, 0);
    CHECK(Count(first) == 1);
    first = restated::Rasterize(nx, ny, nz, res, nullptr, OneSphere(0.0), Pose(0.75, 1.0, 1.25), 1, 0.0, 0);
    CHECK(Count(first) == 0);  // a lattice corner
    first = restated::Rasterize(nx, ny, nz, res, nullptr, OneSphere(0.25), centre, 1, -0.3, 0);
    CHECK(Count(first) == 0);  // R < 0
    first = restated::Rasterize(nx, ny, nz, res, nullptr, OneSphere(0.25), centre, 1, -0.25, 0);
    CHECK(Count(first) == 1);  // R == 0
    // two configurations on one cell: the lower index; base and keep as unsigned minima, in either order
    std::vector<double> poses;
    Append(poses, centre);
    Append(poses, Pose(0.125, 0.125, 0.125));
    Append(poses, centre);
    Append(poses, Pose(0.375, 0.125, 0.125));
    const std::vector<int32_t> whole = restated::Rasterize(nx, ny, nz, res, nullptr, OneSphere(0.0), poses, 1, 0.0, 10);
    CHECK(Count(whole) == 3 && at(whole, 3, 4, 5) == 10 && at(whole, 0, 0, 0) == 11 && at(whole, 1, 0, 0) == 13);
    const std::vector<double> low(poses.begin(), poses.begin() + 32), high(poses.begin() + 32, poses.end());
    std::vector<int32_t> a = restated::Rasterize(nx, ny, nz, res, nullptr, OneSphere(0.0), low, 1, 0.0, 10);
    a = restated::Rasterize(nx, ny, nz, res, nullptr, OneSphere(0.0), high, 1, 0.0, 12, &a);
    std::vector<int32_t> b = restated::Rasterize(nx, ny, nz, res, nullptr, OneSphere(0.0), high, 1, 0.0, 12);
    CHECK(at(b, 3, 4, 5) == 12 && at(b, 0, 0, 0) == -1);
    b = restated::Rasterize(nx, ny, nz, res, nullptr, OneSphere(0.0), low, 1, 0.0, 10, &b);
    CHECK(a == whole && b == whole);
    // not usable: non-finite pose entries, a link out of range
    std::vector<double> bad = centre;
    bad[12] = nan;
    CHECK(Count(restated::Rasterize(nx, ny, nz, res, nullptr, OneSphere(5.0), bad, 1, 0.0, 0)) == 0);
    bad = centre;
    bad[13] = inf;
    CHECK(Count(restated::Rasterize(nx, ny, nz, res, nullptr, OneSphere(5.0), bad, 1, 0.0, 0)) == 0);
    SphereModel elsewhere = OneSphere(5.0);
    elsewhere.link = {1};
    CHECK(Count(restated::Rasterize(nx, ny, nz, res, nullptr, elsewhere, centre, 1, 0.0, 0)) == 0);
    CHECK(Count(restated::Rasterize(nx, ny, nz, res, nullptr, OneSphere(5.0), centre, 1, 0.0, 0)) == nx * ny * nz);
    // under a grid_from_world: c = w + (-1, 0, 0.25)
    const std::vector<double> M = Pose(-1.0, 0.0, 0.25);
    first = restated::Rasterize(nx, ny, nz, res, M.data(), OneSphere(0.0), Pose(1.875, 1.125, 1.125), 1, 0.0, 0);
    CHECK(Count(first) == 1 && at(first, 3, 4, 5) == 0);
    // points: the least (b, s); the filtered cloud keeps the bits
    SphereModel three;
    three.link = {0, 1, 0};
    three.xyzr = {{{0.0, 0.0, 0.0, 0.25}}, {{0.0, 0.0, 0.0, 1.0}}, {{0.5, 0.0, 0.0, 0.0}}};
    std::vector<double> two;
    Append(two, Pose(1, 1, 1));
    Append(two, Pose(9, 9, 9));
    Append(two, Pose(3, 3, 3));
    Append(two, Pose(1, 1, 1));
    const float fnan = std::numeric_limits<float>::quiet_NaN(), finf = std::numeric_limits<float>::infinity();
    const std::vector<float> points = {1.0f, 1.0f, 1.25f, 1.0f, 1.5f, 1.0f, 1.5f, 1.0f, 1.0f, -0.0f, 5.0f, -3.0f,
                                       fnan, 1.0f, 1.0f,  1.0f, finf, 1.0f, 3.5f, 3.0f, 3.0f};
    const PointsOnSphereModel got = restated::Cover(points, nullptr, three, two, 2, 0.0);
    CHECK(got.first_configuration == (std::vector<int32_t>{0, 1, 0, -1, -1, -1, 1}));
    CHECK(got.first_sphere == (std::vector<int32_t>{0, 1, 2, -1, -1, -1, 2}));
    CHECK(std::isnan(got.filtered[0]) && std::isnan(got.filtered[8]) && std::isnan(got.filtered[20]));
    CHECK(std::memcmp(&got.filtered[9], &points[9], 9 * sizeof(float)) == 0 && std::signbit(got.filtered[9]));
    std::vector<float> shifted = points;
    for (size_t i = 0; i < shifted.size(); i += 3) shifted[i] -= 1.0f;
    const std::vector<double> T = Pose(1.0, 0.0, 0.0);
    const PointsOnSphereModel moved = restated::Cover(shifted, T.data(), three, two, 2, 0.0);
    CHECK(moved.first_configuration == got.first_configuration && moved.first_sphere == got.first_sphere);
  }

  // argument errors of the layer, raised before a device is asked for
  const SphereModel model = OneSphere(0.25);
  const Isometry3 identity = Isometry3::Identity();
  SphereVolumeOptions options;
  CHECK(ThrowsInvalidArgument([&] { RasterizeSphereModel(-1, 4, 4, res, identity, model, centre, 1); }, "negative"));
  CHECK(ThrowsInvalidArgument([&] { RasterizeSphereModel(4, 4, 4, 0.0, identity, model, centre, 1); }, "resolution"));
  CHECK(ThrowsInvalidArgument([&] { RasterizeSphereModel(2048, 1024, 1024, res, identity, model, centre, 1); }, "2^31"));
  CHECK(ThrowsInvalidArgument([&] { RasterizeSphereModel(4, 4, 4, res, identity, model, centre, -1); }, "negative"));
  CHECK(ThrowsInvalidArgument([&] { RasterizeSphereModel(4, 4, 4, res, identity, model, {}, 0); }, "num_links == 0"));
  CHECK(ThrowsInvalidArgument([&] { RasterizeSphereModel(4, 4, 4, res, identity, model, std::vector<double>(17, 0.0), 1); },
                              "per configuration"));
  options.padding = nan;
  CHECK(ThrowsInvalidArgument([&] { RasterizeSphereModel(4, 4, 4, res, identity, model, centre, 1, options); }, "padding"));
  options = SphereVolumeOptions();
  options.first_configuration_base = -1;
  CHECK(ThrowsInvalidArgument([&] { RasterizeSphereModel(4, 4, 4, res, identity, model, centre, 1, options); },
                              "first_configuration_base"));
  options.first_configuration_base = 0x7fffffffLL;
  CHECK(ThrowsInvalidArgument([&] { RasterizeSphereModel(4, 4, 4, res, identity, model, centre, 1, options); },
                              "first_configuration_base"));
  options = SphereVolumeOptions();
  {
    SphereModel bad = model;
    bad.link = {1};
    CHECK(ThrowsInvalidArgument([&] { RasterizeSphereModel(4, 4, 4, res, identity, bad, centre, 1); }, "sphere 0: link 1"));
    bad = model;
    bad.xyzr[0][3] = -0.5;
    CHECK(ThrowsInvalidArgument([&] { RasterizeSphereModel(4, 4, 4, res, identity, bad, centre, 1); },
                                "sphere 0: the radius"));
    CHECK(ThrowsInvalidArgument([&] { FindPointsOnSphereModel({0.0f, 0.0f, 0.0f}, identity, bad, centre, 1); },
                                "sphere 0: the radius"));
    bad = model;
    bad.link.push_back(0);
    CHECK(ThrowsInvalidArgument([&] { RasterizeSphereModel(4, 4, 4, res, identity, bad, centre, 1); }, "one link"));
    const std::vector<int32_t> short_keep(5, -1);
    CHECK(ThrowsInvalidArgument([&] { RasterizeSphereModel(4, 4, 4, res, identity, model, centre, 1, options, &short_keep); },
                                "keep"));
    CHECK(ThrowsInvalidArgument([&] { FindPointsOnSphereModel({0.0f, 0.0f}, identity, model, centre, 1); }, "three floats"));
    OccupancyMap none;
    CHECK(ThrowsInvalidArgument([&] { RasterizeSphereModelIntoOccupancyMap(none, model, centre, 1); }, "initialized"));
    OccupancyMap map(identity, "f", res, 4, 4, 4, 0.0f);
    SphereOccupancyOptions keep_nothing;
    keep_nothing.keep = true;
    CHECK(ThrowsInvalidArgument([&] { RasterizeSphereModelIntoOccupancyMap(map, model, centre, 1, keep_nothing); }, "keep"));
  }
  // nothing to cover with: no device is needed
  {
    const std::vector<int32_t> none = RasterizeSphereModel(4, 3, 2, res, identity, model, {}, 1);
    CHECK(none == std::vector<int32_t>(24, -1));
    const std::vector<int32_t> kept(24, 7);
    CHECK(RasterizeSphereModel(4, 3, 2, res, identity, SphereModel(), centre, 1, options, &kept) == kept);
    CHECK(RasterizeSphereModel(4, 0, 2, res, identity, model, centre, 1).empty());
    OccupancyMap map(identity, "f", res, 4, 3, 2, 0.25f);
    std::vector<int32_t> first;
    SphereOccupancyOptions into;
    into.first_configuration = &first;
    CHECK(RasterizeSphereModelIntoOccupancyMap(map, model, {}, 1, into) == 0 && first == std::vector<int32_t>(24, -1));
    CHECK(map.GetIndexImmutable(1, 1, 1) == 0.25f);
    const std::vector<float> points = {1.0f, 2.0f, 3.0f, -0.0f, std::numeric_limits<float>::quiet_NaN(), 5.0f};
    const PointsOnSphereModel plain = FindPointsOnSphereModel(points, identity, model, {}, 1);
    CHECK(plain.first_configuration == std::vector<int32_t>(2, -1) && plain.first_sphere == std::vector<int32_t>(2, -1));
    CHECK(SameBytes(plain.filtered, points));
    PointsOnSphereModelOptions brief;
    brief.filtered = false;
    CHECK(FindPointsOnSphereModel(points, identity, SphereModel(), centre, 1, brief).filtered.empty());
    CHECK(FindPointsOnSphereModel({}, identity, model, centre, 1).first_configuration.empty());
  }

  // the C ABI's own errors, before the context is looked at
  {
    int32_t first[64];
    for (int32_t& v : first) v = 9;
    vgt_hip_ctx* stand_in = reinterpret_cast<vgt_hip_ctx*>(&first);
    const double xyzr[8] = {0, 0, 0, 0.25, 0, 0, 0, -1.0};
    const int32_t link[2] = {0, 1};
    std::vector<double> poses = centre;
    Append(poses, centre);
    auto grid = [&](vgt_hip_ctx* ctx, int64_t n, double r, double padding, int64_t base, uint32_t flags, int64_t links,
                    int32_t* out) {
      return vgt_hip_rasterize_spheres(ctx, n, 4, 4, r, nullptr, xyzr, link, 2, poses.data(), links, 1, padding, base,
                                       flags, out);
    };
    CHECK(grid(nullptr, 4, 1.0, 0.0, 0, 0u, 2, first) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "null") != nullptr);
    CHECK(grid(stand_in, 4, 1.0, 0.0, 0, 0u, 2, nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "null") != nullptr);
    CHECK(grid(stand_in, -4, 1.0, 0.0, 0, 0u, 2, first) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "negative") != nullptr);
    CHECK(grid(stand_in, int64_t{1} << 31, 1.0, 0.0, 0, 0u, 2, first) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "2^31") != nullptr);
    CHECK(grid(stand_in, 4, 0.0, 0.0, 0, 0u, 2, first) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "resolution") != nullptr);
    CHECK(grid(stand_in, 4, 1.0, inf, 0, 0u, 2, first) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "padding") != nullptr);
    CHECK(grid(stand_in, 4, 1.0, 0.0, -1, 0u, 2, first) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "first_configuration_base") != nullptr);
    CHECK(grid(stand_in, 4, 1.0, 0.0, 0, 2u, 2, first) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "flag") != nullptr);
    CHECK(grid(stand_in, 4, 1.0, 0.0, 0, 0u, 0, first) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "num_links == 0") != nullptr);
    CHECK(grid(stand_in, 4, 1.0, 0.0, 0, 0u, 1, first) == VGT_HIP_ERR_INVALID_ARGUMENT);  // link 1 of one link
    CHECK(std::strstr(vgt_hip_last_error(), "sphere 1: link") != nullptr);
    CHECK(grid(stand_in, 4, 1.0, 0.0, 0, 0u, 2, first) == VGT_HIP_ERR_INVALID_ARGUMENT);  // then its radius
    CHECK(std::strstr(vgt_hip_last_error(), "sphere 1: the radius") != nullptr);
    const float points[3] = {0.0f, 0.0f, 0.0f};
    CHECK(vgt_hip_spheres_cover_points(stand_in, points, 1, nullptr, xyzr, link, 2, poses.data(), 2, 1, 0.0, 0u, nullptr,
                                       nullptr, nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "null") != nullptr);
    CHECK(vgt_hip_spheres_cover_points(stand_in, points, 1, nullptr, xyzr, link, 2, poses.data(), 2, 1, 0.0, 1u, first,
                                       nullptr, nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "flag") != nullptr);
    CHECK(vgt_hip_spheres_cover_points(stand_in, points, 1, nullptr, xyzr, link, 2, poses.data(), 2, 1, 0.0, 0u, first,
                                       nullptr, nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "sphere 1: the radius") != nullptr);
    for (int32_t v : first) CHECK(v == 9);
  }
  return g_failures;
}

// A strided float cloud behind the wrapper interface, under an origin transform.
class VectorCloud : public PointCloudWrapper
{
public:
  VectorCloud(const std::vector<float>& points, const Isometry3& origin) : points_(points), origin_(origin) {}
  double MaxRange() const override { return std::numeric_limits<double>::infinity(); }
  int64_t Size() const override { return static_cast<int64_t>(points_.size() / 3); }
  const Isometry3& PointCloudOriginTransform() const override { return origin_; }

private:
  void CopyPointLocationIntoFloatPtrImpl(int64_t point_index, float* destination) const override
  {
    std::memcpy(destination, points_.data() + 3 * point_index, 3 * sizeof(float));
  }
  std::vector<float> points_;
  Isometry3 origin_;
};

static int RunDevice()
{
  uint64_t state = 4321;
  auto next = [&]() {  // uniform in [0, 1)
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<double>(state >> 11) * (1.0 / 9007199254740992.0);
  };
  // 13 x 11 x 9 at 0.125 under an origin transform; 70 spheres on 5 links, 37 configurations
  const Isometry3 origin = Isometry3::FromQuaternion(std::cos(0.2), 0.0, 0.0, std::sin(0.2), 0.3, -0.2, 0.1);
  const int64_t nx = 13, ny = 11, nz = 9;
  const double res = 0.125;
  SphereModel model;
  for (int s = 0; s < 70; s++)
  {
    model.link.push_back(static_cast<int32_t>(next() * 5.0) % 5);
    model.xyzr.push_back({{next() * 0.4 - 0.2, next() * 0.4 - 0.2, next() * 0.4 - 0.2, s % 4 == 0 ? 0.0 : next() * 0.15}});
  }
  std::vector<double> poses;
  for (int b = 0; b < 37; b++)
    for (int k = 0; k < 5; k++)
    {
      const double angle = next() * 6.0;
      const Isometry3 in_grid = Isometry3::FromQuaternion(std::cos(angle), std::sin(angle) * 0.6, 0.0, std::sin(angle) * 0.8,
                                                          next() * 2.0 - 0.2, next() * 1.7 - 0.2, next() * 1.5 - 0.2);
      const Isometry3 pose = origin * in_grid;
      poses.insert(poses.end(), pose.m.begin(), pose.m.end());
    }
  poses[16 * 7 + 13] = std::numeric_limits<double>::quiet_NaN();
  poses[16 * 11 + 4] = std::numeric_limits<double>::infinity();
  const Isometry3 grid_from_world = origin.Inverse();

  for (const double padding : {0.0, 0.05, -0.04})
  {
    SphereVolumeOptions options;
    options.padding = padding;
    options.first_configuration_base = 100;
    const std::vector<int32_t> want =
        restated::Rasterize(nx, ny, nz, res, grid_from_world.m.data(), model, poses, 5, padding, 100);
    const std::vector<int32_t> got = RasterizeSphereModel(nx, ny, nz, res, origin, model, poses, 5, options);
    std::printf("padding %g: %lld of %lld cells covered\n", padding, static_cast<long long>(Count(want)),
                static_cast<long long>(nx * ny * nz));
    CHECK(Count(want) > 0 && Count(want) < nx * ny * nz && SameBytes(got, want));
    // in two pieces, the later one first
    const size_t cut = 12 * 5 * 16;
    const std::vector<double> low(poses.begin(), poses.begin() + cut), high(poses.begin() + cut, poses.end());
    options.first_configuration_base = 112;
    const std::vector<int32_t> later = RasterizeSphereModel(nx, ny, nz, res, origin, model, high, 5, options);
    options.first_configuration_base = 100;
    CHECK(SameBytes(RasterizeSphereModel(nx, ny, nz, res, origin, model, low, 5, options, &later), want));

    // into an occupancy map: covered cells filled, the rest as they were
    OccupancyMap map(origin, "f", res, nx, ny, nz, 0.0f);
    for (int64_t x = 0; x < nx; x++)
      for (int64_t y = 0; y < ny; y++)
        for (int64_t z = 0; z < nz; z++) map.SetIndex(x, y, z, static_cast<float>((x + 2 * y + 3 * z) % 7) * 0.125f);
    const OccupancyMap before = map;
    std::vector<int32_t> first;
    SphereOccupancyOptions into;
    into.padding = padding;
    into.first_configuration_base = 100;
    into.filled_value = 2.0f;
    into.first_configuration = &first;
    CHECK(RasterizeSphereModelIntoOccupancyMap(map, model, poses, 5, into) == Count(want) && SameBytes(first, want));
    bool as_expected = true;
    for (size_t i = 0; i < want.size(); i++)
      as_expected = as_expected && map.GetImmutableRawData()[i] == (want[i] >= 0 ? 2.0f : before.GetImmutableRawData()[i]);
    CHECK(as_expected);

    // points: in a sensor frame, near the spheres and elsewhere, some not finite
    const Isometry3 world_from_points = Isometry3::FromQuaternion(std::cos(0.4), 0.0, std::sin(0.4), 0.0, 0.5, 0.2, -0.1);
    const Isometry3 points_from_world = world_from_points.Inverse();
    std::vector<float> points;
    for (int i = 0; i < 700; i++)
    {
      const size_t b = static_cast<size_t>(next() * 37.0) % 37, s = static_cast<size_t>(next() * 70.0) % 70;
      const restated::Sphere sphere = restated::Place(model, poses, 5, b, s, padding, nullptr);
      double w[3];
      for (int a = 0; a < 3; a++)
        w[a] = (i % 2 == 0 && sphere.usable) ? sphere.c[a] + (next() - 0.5) * 0.2 : next() * 2.4 - 0.4;
      for (int r = 0; r < 3; r++)
        points.push_back(static_cast<float>(points_from_world(r, 0) * w[0] + points_from_world(r, 1) * w[1] +
                                            points_from_world(r, 2) * w[2] + points_from_world(r, 3)));
    }
    points[3 * 5] = std::numeric_limits<float>::quiet_NaN();
    points[3 * 9 + 1] = std::numeric_limits<float>::infinity();
    points[3 * 11 + 2] = -0.0f;
    const PointsOnSphereModel want_points = restated::Cover(points, world_from_points.m.data(), model, poses, 5, padding);
    const PointsOnSphereModel got_points = FindPointsOnSphereModel(points, world_from_points, model, poses, 5,
                                                                   PointsOnSphereModelOptions{padding, true, 0});
    int64_t covered = 0;
    for (int32_t v : want_points.first_configuration) covered += v >= 0;
    std::printf("padding %g: %lld of 700 points covered\n", padding, static_cast<long long>(covered));
    CHECK(covered > 0 && covered < 700);
    CHECK(SameBytes(got_points.first_configuration, want_points.first_configuration));
    CHECK(SameBytes(got_points.first_sphere, want_points.first_sphere));
    CHECK(SameFloats(got_points.filtered, want_points.filtered));
    const PointsOnSphereModel through_wrapper =
        FindPointsOnSphereModel(VectorCloud(points, world_from_points), model, poses, 5,
                                PointsOnSphereModelOptions{padding, false, 0});
    CHECK(SameBytes(through_wrapper.first_configuration, want_points.first_configuration));
    CHECK(SameBytes(through_wrapper.first_sphere, want_points.first_sphere) && through_wrapper.filtered.empty());
  }
  return g_failures;
}

int main(int argc, char** argv)
{
  const bool no_device = argc > 1 && std::strcmp(argv[1], "--no-device") == 0;
  int failures = RunNoDevice();
  if (!no_device) failures = RunDevice();
  if (failures == 0) std::printf("PASSED\n");
  return failures == 0 ? 0 : 1;
}
