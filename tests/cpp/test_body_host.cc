// CheckSphereModel of the C++ host layer (include/vgt_hip/body_queries.hpp) against an in-file restatement of
// vgt_hip_check_spheres (include/vgt_hip.h), bit for bit.
//   test_body_host              the restatement against hand-derived answers, the argument errors, and the layer on
//                               device 0 against the restatement
//   test_body_host --no-device  the first two only: nothing here touches a device
#include <vgt_hip.h>
#include <vgt_hip/body_queries.hpp>

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

// ---- the restatement: every step in the order include/vgt_hip.h gives, one sphere at a time ----
namespace restated
{
const double kNaN = std::numeric_limits<double>::quiet_NaN();

struct Cell
{
  double g[3];
  int64_t i[3], lo[3], hi[3];
};

static void AxisIndices(int64_t initial, int64_t size, double offset, int64_t& lower, int64_t& upper)
{
  lower = upper = initial;
  if (offset >= 0.0)
  {
    upper = initial + 1;
    if (upper >= size)
    {
      upper = initial;
      lower = initial - 1;
      if (lower < 0) lower = initial;
    }
  }
  else
  {
    lower = initial - 1;
    if (lower < 0)
    {
      upper = initial + 1;
      lower = initial;
      if (upper >= size) upper = initial;
    }
  }
}

static bool Locate(const DenseGrid& grid, const double w[3], Cell& c)
{
  const auto& M = grid.InverseOriginTransform().m;
  const double res = grid.Resolution(), inv = 1.0 / res;
  const int64_t n[3] = {grid.NumXVoxels(), grid.NumYVoxels(), grid.NumZVoxels()};
  for (int r = 0; r < 3; r++) c.g[r] = M[r] * w[0] + M[4 + r] * w[1] + M[8 + r] * w[2] + M[12 + r];
  for (int r = 0; r < 3; r++)
  {
    const double f = std::floor(c.g[r] * inv);
    if (!(f >= 0.0 && f < static_cast<double>(n[r]))) return false;
    c.i[r] = static_cast<int64_t>(f);
  }
  for (int r = 0; r < 3; r++)
    AxisIndices(c.i[r], n[r], c.g[r] - (static_cast<double>(c.i[r]) + 0.5) * res, c.lo[r], c.hi[r]);
  return true;
}

static double Corrected(const DenseGrid& grid, int64_t x, int64_t y, int64_t z)
{
  const double nominal = static_cast<double>(grid.GetIndexImmutable(x, y, z));
  const double offset = grid.Resolution() * 0.5;
  return nominal >= 0.0 ? nominal - offset : nominal + offset;
}

static double Lerp(double a, double b, double t) { return a * (1.0 - t) + b * t; }

static double Estimate(const DenseGrid& grid, const Cell& c)
{
  const double res = grid.Resolution();
  double t[3];
  for (int r = 0; r < 3; r++)
  {
    const double low = (static_cast<double>(c.lo[r]) + 0.5) * res;
    t[r] = (c.g[r] - low) / ((low + res) - low);
  }
  const double mm = Lerp(Corrected(grid, c.lo[0], c.lo[1], c.lo[2]), Corrected(grid, c.hi[0], c.lo[1], c.lo[2]), t[0]);
  const double mp = Lerp(Corrected(grid, c.lo[0], c.lo[1], c.hi[2]), Corrected(grid, c.hi[0], c.lo[1], c.hi[2]), t[0]);
  const double pm = Lerp(Corrected(grid, c.lo[0], c.hi[1], c.lo[2]), Corrected(grid, c.hi[0], c.hi[1], c.lo[2]), t[0]);
  const double pp = Lerp(Corrected(grid, c.lo[0], c.hi[1], c.hi[2]), Corrected(grid, c.hi[0], c.hi[1], c.hi[2]), t[0]);
  return Lerp(Lerp(mm, pm, t[1]), Lerp(mp, pp, t[1]), t[2]);
}

// the coarse gradient with edge gradients, rotated by the origin transform's rotation
static void Gradient(const DenseGrid& grid, const Cell& c, double out[3])
{
  const double res = grid.Resolution();
  const int64_t n[3] = {grid.NumXVoxels(), grid.NumYVoxels(), grid.NumZVoxels()};
  const int64_t x = c.i[0], y = c.i[1], z = c.i[2];
  auto at = [&](int axis, int64_t k) {
    int64_t p[3] = {x, y, z};
    p[axis] = k;
    return grid.GetIndexImmutable(p[0], p[1], p[2]);
  };
  double g[3] = {0.0, 0.0, 0.0};
  const bool interior = x > 0 && y > 0 && z > 0 && x < n[0] - 1 && y < n[1] - 1 && z < n[2] - 1;
  for (int a = 0; a < 3; a++)
  {
    const int64_t k = c.i[a];
    if (interior)
    {
      g[a] = static_cast<double>(at(a, k + 1) - at(a, k - 1)) * (1.0 / (2.0 * res));  // (the difference in float)
    }
    else
    {
      const int64_t lo = k - 1 < 0 ? 0 : k - 1, hi = k + 1 > n[a] - 1 ? n[a] - 1 : k + 1;
      const double increment = static_cast<double>(hi - lo) * res;
      if (increment > 0.0)
        g[a] = (static_cast<double>(at(a, hi)) - static_cast<double>(at(a, lo))) * (1.0 / increment);
    }
  }
  const Isometry3& o = grid.OriginTransform();
  for (int r = 0; r < 3; r++) out[r] = o(r, 0) * g[0] + o(r, 1) * g[1] + o(r, 2) * g[2];
}

static SphereModelChecks Check(const SignedDistanceField& sdf, const SphereModel& model, const std::vector<double>& poses,
                               int64_t num_links, double minimum_clearance, bool outside_is_collision)
{
  const DenseGrid& grid = sdf.grid;
  const size_t s_count = model.link.size();
  const size_t b_count = poses.size() / (static_cast<size_t>(num_links) * 16);
  SphereModelChecks out;
  for (size_t b = 0; b < b_count; b++)
  {
    int32_t below = 0, outside = 0, best = -1;
    double best_clearance = kNaN, best_gradient[3] = {kNaN, kNaN, kNaN};
    for (size_t s = 0; s < s_count; s++)
    {
      const double* m = poses.data() + (b * static_cast<size_t>(num_links) + static_cast<size_t>(model.link[s])) * 16;
      const double x = model.xyzr[s][0], y = model.xyzr[s][1], z = model.xyzr[s][2];
      double w[3];
      for (int r = 0; r < 3; r++) w[r] = ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r];
      Cell c;
      double clearance = kNaN, gradient[3] = {kNaN, kNaN, kNaN};
      if (Locate(grid, w, c))
      {
        clearance = Estimate(grid, c) - model.xyzr[s][3];
        Gradient(grid, c, gradient);
        if (clearance <= minimum_clearance) below++;
        if (best < 0 ? clearance == clearance : clearance < best_clearance)
        {
          best = static_cast<int32_t>(s);
          best_clearance = clearance;
          for (int r = 0; r < 3; r++) best_gradient[r] = gradient[r];
        }
      }
      else
      {
        outside++;
      }
      out.sphere_clearance.push_back(clearance);
      for (int r = 0; r < 3; r++) out.sphere_gradient.push_back(gradient[r]);
    }
    uint8_t status = VGT_HIP_SPHERES_NO_VALUE;
    if (below > 0 || (outside_is_collision && outside > 0))
      status = VGT_HIP_SPHERES_COLLISION;
    else if (best >= 0)
      status = VGT_HIP_SPHERES_CLEAR;
    out.status.push_back(status);
    out.min_clearance.push_back(best_clearance);
    out.min_sphere.push_back(best);
    out.num_below.push_back(below);
    out.num_outside.push_back(outside);
    for (int r = 0; r < 3; r++) out.min_gradient.push_back(best_gradient[r]);
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

// 4 x 4 x 4 at resolution 1, the value of a cell its x index: the estimate at the centre of cell (i, j, k) is i - 0.5
// (cell 0: -0.5), the gradient (1, 0, 0) everywhere
static SignedDistanceField Ramp(const Isometry3& origin)
{
  SignedDistanceField sdf;
  sdf.grid = DenseGrid(origin, "f", 1.0, 4, 4, 4, 0.0f);
  for (int64_t x = 0; x < 4; x++)
    for (int64_t y = 0; y < 4; y++)
      for (int64_t z = 0; z < 4; z++) sdf.grid.SetIndex(x, y, z, static_cast<float>(x));
  return sdf;
}

// spheres 0 and 2 (a copy) on link 0 with radius 0.25, sphere 1 on link 1 with radius 0
static SphereModel ThreeSpheres()
{
  SphereModel model;
  model.link = {0, 1, 0};
  model.xyzr = {{{0.0, 0.0, 0.0, 0.25}}, {{0.0, 0.0, 0.0, 0.0}}, {{0.0, 0.0, 0.0, 0.25}}};
  return model;
}

static std::vector<double> ThreeConfigurations()
{
  std::vector<double> poses;
  Append(poses, Pose(1.5, 1.5, 1.5));  // clearances 0.25, 1.5, 0.25
  Append(poses, Pose(2.5, 1.5, 1.5));
  Append(poses, Pose(-1.0, 1.5, 1.5));  // -, 2.5, -
  Append(poses, Pose(3.5, 0.5, 0.5));
  Append(poses, Pose(1.5, 4.5, 1.5));  // -, -, -
  Append(poses, Pose(1.5, 1.5, -0.5));
  return poses;
}

static int RunNoDevice()
{
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const SignedDistanceField sdf = Ramp(Isometry3::Identity());
  const SphereModel model = ThreeSpheres();
  const std::vector<double> poses = ThreeConfigurations();

  // the restatement against answers derived by hand
  {
    const SphereModelChecks got = restated::Check(sdf, model, poses, 2, 0.0, false);
    CHECK(got.status == (std::vector<uint8_t>{VGT_HIP_SPHERES_CLEAR, VGT_HIP_SPHERES_CLEAR, VGT_HIP_SPHERES_NO_VALUE}));
    CHECK(got.min_sphere == (std::vector<int32_t>{0, 1, -1}));  // (0, not its copy 2)
    CHECK(got.num_below == (std::vector<int32_t>{0, 0, 0}) && got.num_outside == (std::vector<int32_t>{0, 2, 3}));
    CHECK(got.min_clearance[0] == 0.25 && got.min_clearance[1] == 2.5 && std::isnan(got.min_clearance[2]));
    CHECK(got.min_gradient[0] == 1.0 && got.min_gradient[1] == 0.0 && got.min_gradient[2] == 0.0);
    CHECK(got.min_gradient[3] == 1.0 && std::isnan(got.min_gradient[6]) && std::isnan(got.min_gradient[8]));
    CHECK(got.sphere_clearance[1] == 1.5 && got.sphere_clearance[2] == 0.25 && std::isnan(got.sphere_clearance[3]));
    const SphereModelChecks edge = restated::Check(sdf, model, poses, 2, 0.25, false);  // <=
    CHECK(edge.status[0] == VGT_HIP_SPHERES_COLLISION && edge.num_below[0] == 2 && edge.num_below[1] == 0);
    const SphereModelChecks flagged = restated::Check(sdf, model, poses, 2, 0.0, true);
    CHECK(flagged.status ==
          (std::vector<uint8_t>{VGT_HIP_SPHERES_CLEAR, VGT_HIP_SPHERES_COLLISION, VGT_HIP_SPHERES_COLLISION}));
    // under an origin transform: a quarter turn about z and a shift; the grid's x is the world's y
    const Isometry3 origin = Isometry3::FromQuaternion(std::sqrt(0.5), 0.0, 0.0, std::sqrt(0.5), 10.0, 20.0, 30.0);
    const SignedDistanceField turned = Ramp(origin);
    SphereModel one;
    one.link = {0};
    one.xyzr = {{{0.0, 0.0, 0.0, 0.5}}};
    // the centre of cell (2, 0, 3): grid (2.5, 0.5, 3.5) -> world (10 - 0.5, 20 + 2.5, 30 + 3.5)
    const SphereModelChecks world = restated::Check(turned, one, Pose(9.5, 22.5, 33.5), 1, 0.0, false);
    CHECK(world.status[0] == VGT_HIP_SPHERES_CLEAR && std::abs(world.min_clearance[0] - 1.0) < 1e-12);
    CHECK(std::abs(world.min_gradient[0]) < 1e-12 && std::abs(world.min_gradient[1] - 1.0) < 1e-12);
  }

  // argument errors of the layer, raised before a device is asked for
  CHECK(ThrowsInvalidArgument([&] { CheckSphereModel(SignedDistanceField(), model, poses, 2); }, "initialized"));
  SphereModelOptions options;
  options.minimum_clearance = nan;
  CHECK(ThrowsInvalidArgument([&] { CheckSphereModel(sdf, model, poses, 2, options); }, "minimum_clearance"));
  CHECK(ThrowsInvalidArgument([&] { CheckSphereModel(sdf, model, poses, -1); }, "negative"));
  CHECK(ThrowsInvalidArgument([&] { CheckSphereModel(sdf, model, {}, 0); }, "num_links == 0"));
  CHECK(ThrowsInvalidArgument([&] { CheckSphereModel(sdf, model, poses, 1); }, "sphere 1: link 1"));
  CHECK(ThrowsInvalidArgument([&] { CheckSphereModel(sdf, model, std::vector<double>(33, 0.0), 2); }, "per configuration"));
  {
    SphereModel bad = model;
    bad.xyzr[2][3] = -0.5;
    CHECK(ThrowsInvalidArgument([&] { CheckSphereModel(sdf, bad, poses, 2); }, "sphere 2: the radius"));
    bad.xyzr[2][3] = nan;
    CHECK(ThrowsInvalidArgument([&] { CheckSphereModel(sdf, bad, poses, 2); }, "sphere 2: the radius"));
    bad = model;
    bad.link.pop_back();
    CHECK(ThrowsInvalidArgument([&] { CheckSphereModel(sdf, bad, poses, 2); }, "one link"));
  }
  // nothing to compare: no device is needed
  {
    const SphereModelChecks none = CheckSphereModel(sdf, model, {}, 2);
    CHECK(none.status.empty() && none.min_clearance.empty() && none.min_gradient.empty() && none.sphere_clearance.empty());
    options = SphereModelOptions();
    options.per_sphere = true;
    options.outside_is_collision = true;
    const SphereModelChecks no_spheres = CheckSphereModel(sdf, SphereModel(), poses, 2, options);
    CHECK(no_spheres.status == std::vector<uint8_t>(3, VGT_HIP_SPHERES_NO_VALUE));
    CHECK(no_spheres.min_sphere == std::vector<int32_t>(3, -1) && no_spheres.num_outside == std::vector<int32_t>(3, 0));
    CHECK(std::isnan(no_spheres.min_clearance[2]) && std::isnan(no_spheres.min_gradient[8]));
    CHECK(no_spheres.sphere_clearance.empty() && no_spheres.sphere_gradient.empty());
  }

  // the C ABI's own errors, before the context is looked at
  {
    uint8_t status[3] = {9, 9, 9};
    const float field[64] = {};
    vgt_hip_ctx* stand_in = reinterpret_cast<vgt_hip_ctx*>(&status);
    const double xyzr[12] = {0, 0, 0, 0.25, 0, 0, 0, -1.0, 0, 0, 0, 0.25};
    const int32_t link[3] = {0, 1, 0};
    auto call = [&](vgt_hip_ctx* ctx, int64_t nx, double res, double clearance, uint32_t flags, int64_t links,
                    uint8_t* st) {
      return vgt_hip_check_spheres(ctx, field, nx, 4, 4, res, nullptr, nullptr, xyzr, link, 3, poses.data(), links, 3,
                                   clearance, flags, st, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    };
    CHECK(call(nullptr, 4, 1.0, 0.0, 0u, 2, status) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "null") != nullptr);
    CHECK(call(stand_in, 4, 1.0, 0.0, 0u, 2, nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "null") != nullptr);
    CHECK(call(stand_in, -4, 1.0, 0.0, 0u, 2, status) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "negative") != nullptr);
    CHECK(call(stand_in, int64_t{1} << 31, 1.0, 0.0, 0u, 2, status) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "2^31") != nullptr);
    CHECK(call(stand_in, 4, 0.0, 0.0, 0u, 2, status) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "resolution") != nullptr);
    CHECK(call(stand_in, 4, 1.0, nan, 0u, 2, status) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "minimum_clearance") != nullptr);
    CHECK(call(stand_in, 4, 1.0, 0.0, 2u, 2, status) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "flag") != nullptr);
    CHECK(call(stand_in, 4, 1.0, 0.0, 0u, 0, status) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "num_links == 0") != nullptr);
    CHECK(call(stand_in, 4, 1.0, 0.0, 0u, 1, status) == VGT_HIP_ERR_INVALID_ARGUMENT);  // link 1 of one link: sphere 1
    CHECK(std::strstr(vgt_hip_last_error(), "sphere 1: link") != nullptr);
    CHECK(call(stand_in, 4, 1.0, 0.0, 0u, 2, status) == VGT_HIP_ERR_INVALID_ARGUMENT);  // then its radius
    CHECK(std::strstr(vgt_hip_last_error(), "sphere 1: the radius") != nullptr);
    CHECK(status[0] == 9 && status[1] == 9 && status[2] == 9);
  }
  return g_failures;
}

template <typename T>
static bool SameBytes(const std::vector<T>& a, const std::vector<T>& b)
{
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// doubles: the same bits, or NaN in both
static bool SameDoubles(const std::vector<double>& a, const std::vector<double>& b)
{
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (!(std::isnan(a[i]) && std::isnan(b[i])) && std::memcmp(&a[i], &b[i], sizeof(double)) != 0) return false;
  return true;
}

static void CheckAgainstRestatement(const SignedDistanceField& sdf, const SphereModel& model,
                                    const std::vector<double>& poses, int64_t num_links, double minimum_clearance,
                                    bool outside_is_collision)
{
  SphereModelOptions options;
  options.minimum_clearance = minimum_clearance;
  options.outside_is_collision = outside_is_collision;
  options.per_sphere = true;
  const SphereModelChecks got = CheckSphereModel(sdf, model, poses, num_links, options);
  const SphereModelChecks want = restated::Check(sdf, model, poses, num_links, minimum_clearance, outside_is_collision);
  CHECK(SameBytes(got.status, want.status) && SameBytes(got.min_sphere, want.min_sphere));
  CHECK(SameBytes(got.num_below, want.num_below) && SameBytes(got.num_outside, want.num_outside));
  CHECK(SameDoubles(got.min_clearance, want.min_clearance) && SameDoubles(got.min_gradient, want.min_gradient));
  CHECK(SameDoubles(got.sphere_clearance, want.sphere_clearance));
  CHECK(SameDoubles(got.sphere_gradient, want.sphere_gradient));
  options.per_sphere = false;
  const SphereModelChecks brief = CheckSphereModel(sdf, model, poses, num_links, options);
  CHECK(brief.sphere_clearance.empty() && brief.sphere_gradient.empty());
  CHECK(SameBytes(brief.status, want.status) && SameDoubles(brief.min_clearance, want.min_clearance));
}

static int RunDevice()
{
  // the hand-derived scene
  {
    const SignedDistanceField sdf = Ramp(Isometry3::Identity());
    SphereModelOptions options;
    const SphereModelChecks got = CheckSphereModel(sdf, ThreeSpheres(), ThreeConfigurations(), 2, options);
    CHECK(got.status == (std::vector<uint8_t>{VGT_HIP_SPHERES_CLEAR, VGT_HIP_SPHERES_CLEAR, VGT_HIP_SPHERES_NO_VALUE}));
    CHECK(got.min_sphere == (std::vector<int32_t>{0, 1, -1}) && got.num_outside == (std::vector<int32_t>{0, 2, 3}));
    CHECK(got.min_clearance[0] == 0.25 && got.min_gradient[0] == 1.0 && got.sphere_clearance.empty());
    CheckAgainstRestatement(sdf, ThreeSpheres(), ThreeConfigurations(), 2, 0.25, false);
    CheckAgainstRestatement(sdf, ThreeSpheres(), ThreeConfigurations(), 2, 0.0, true);
  }
  // a rolling field under an origin transform, 70 spheres on 5 links (two slices), 37 configurations
  {
    const Isometry3 origin = Isometry3::FromQuaternion(std::cos(0.2), 0.0, 0.0, std::sin(0.2), 0.3, -0.2, 0.1);
    SignedDistanceField sdf;
    sdf.grid = DenseGrid(origin, "f", 0.125, 11, 9, 13, 0.0f);
    for (int64_t x = 0; x < 11; x++)
      for (int64_t y = 0; y < 9; y++)
        for (int64_t z = 0; z < 13; z++)
          sdf.grid.SetIndex(x, y, z, static_cast<float>(0.3 * std::sin(0.7 * x) + 0.25 * std::cos(0.9 * y) - 0.1 * z + 0.4));
    sdf.grid.SetIndex(5, 4, 6, std::numeric_limits<float>::quiet_NaN());
    sdf.grid.SetIndex(2, 2, 2, -std::numeric_limits<float>::infinity());
    uint64_t state = 12345;
    auto next = [&]() {  // uniform in [0, 1)
      state = state * 6364136223846793005ull + 1442695040888963407ull;
      return static_cast<double>(state >> 11) * (1.0 / 9007199254740992.0);
    };
    SphereModel model;
    for (int s = 0; s < 70; s++)
    {
      model.link.push_back(static_cast<int32_t>(next() * 5.0) % 5);
      model.xyzr.push_back({{next() * 0.4 - 0.2, next() * 0.4 - 0.2, next() * 0.4 - 0.2, s % 4 == 0 ? 0.0 : next() * 0.1}});
    }
    model.link[69] = model.link[0];
    model.xyzr[69] = model.xyzr[0];
    std::vector<double> poses;
    for (int b = 0; b < 37; b++)
      for (int k = 0; k < 5; k++)
      {
        const double angle = next() * 6.0;
        const Isometry3 in_grid = Isometry3::FromQuaternion(std::cos(angle), std::sin(angle) * 0.6, 0.0, std::sin(angle) * 0.8,
                                                            next() * 1.8 - 0.2, next() * 1.5 - 0.2, next() * 2.0 - 0.2);
        const Isometry3 pose = origin * in_grid;
        poses.insert(poses.end(), pose.m.begin(), pose.m.end());
      }
    poses[16 * 7 + 13] = std::numeric_limits<double>::quiet_NaN();
    poses[16 * 11 + 4] = std::numeric_limits<double>::infinity();
    CheckAgainstRestatement(sdf, model, poses, 5, 0.05, false);
    CheckAgainstRestatement(sdf, model, poses, 5, -0.1, true);
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
