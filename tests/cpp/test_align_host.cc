// AlignPointCloud of the C++ host layer (include/vgt_hip/cloud_alignment.hpp) against an in-file restatement of
// vgt_hip_align_points (include/vgt_hip.h), bit for bit.
//   test_align_host              the restatement against hand-derived answers, the argument errors, and the layer on
//                                device 0 against the restatement
//   test_align_host --no-device  the first two only: nothing here touches a device
#include <vgt_hip.h>
#include <vgt_hip/cloud_alignment.hpp>

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

// ---- the restatement: every step in the order include/vgt_hip.h gives, one point at a time ----
namespace restated
{
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

static double Lerp(double a, double b, double t) { return a * (1.0 - t) + b * t; }

// the estimate and the gradient of its interpolant at w; false: no value
static bool EstimateWithGradient(const DenseGrid& grid, const double w[3], double& d, double g[3])
{
  const auto& M = grid.InverseOriginTransform().m;
  const double res = grid.Resolution(), inv = 1.0 / res;
  const int64_t n[3] = {grid.NumXVoxels(), grid.NumYVoxels(), grid.NumZVoxels()};
  double loc[3], t[3], span[3];
  int64_t lo[3], hi[3];
  for (int r = 0; r < 3; r++) loc[r] = M[r] * w[0] + M[4 + r] * w[1] + M[8 + r] * w[2] + M[12 + r];
  for (int r = 0; r < 3; r++)
  {
    const double f = std::floor(loc[r] * inv);
    if (!(f >= 0.0 && f < static_cast<double>(n[r]))) return false;
    lo[r] = static_cast<int64_t>(f);  // (the cell, until the next loop)
  }
  for (int r = 0; r < 3; r++)
  {
    const int64_t cell = lo[r];
    AxisIndices(cell, n[r], loc[r] - (static_cast<double>(cell) + 0.5) * res, lo[r], hi[r]);
    const double low = (static_cast<double>(lo[r]) + 0.5) * res;
    span[r] = (low + res) - low;
    t[r] = (loc[r] - low) / span[r];
  }
  auto corner = [&](int64_t x, int64_t y, int64_t z) {
    const double nominal = static_cast<double>(grid.GetIndexImmutable(x, y, z));
    const double offset = res * 0.5;
    return nominal >= 0.0 ? nominal - offset : nominal + offset;
  };
  const double mmm = corner(lo[0], lo[1], lo[2]), mmp = corner(lo[0], lo[1], hi[2]), mpm = corner(lo[0], hi[1], lo[2]),
               mpp = corner(lo[0], hi[1], hi[2]), pmm = corner(hi[0], lo[1], lo[2]), pmp = corner(hi[0], lo[1], hi[2]),
               ppm = corner(hi[0], hi[1], lo[2]), ppp = corner(hi[0], hi[1], hi[2]);
  const double tx = t[0], ty = t[1], tz = t[2];
  const double mm = Lerp(mmm, pmm, tx), mp = Lerp(mmp, pmp, tx), pm = Lerp(mpm, ppm, tx), pp = Lerp(mpp, ppp, tx);
  d = Lerp(Lerp(mm, pm, ty), Lerp(mp, pp, ty), tz);
  const double gx = Lerp(Lerp(pmm - mmm, ppm - mpm, ty), Lerp(pmp - mmp, ppp - mpp, ty), tz) / span[0];
  const double gy = Lerp(Lerp(mpm - mmm, ppm - pmm, tx), Lerp(mpp - mmp, ppp - pmp, tx), tz) / span[1];
  const double gz = Lerp(Lerp(mmp - mmm, pmp - pmm, tx), Lerp(mpp - mpm, ppp - ppm, tx), ty) / span[2];
  const Isometry3& o = grid.OriginTransform();
  for (int r = 0; r < 3; r++) g[r] = o(r, 0) * gx + o(r, 1) * gy + o(r, 2) * gz;
  return true;
}

static double TreeSum(std::vector<double> v)
{
  while (true)
  {
    std::vector<double> sums;
    for (size_t first = 0; first < v.size(); first += 64)
    {
      double group[64];
      for (size_t i = 0; i < 64; i++) group[i] = first + i < v.size() ? v[first + i] : 0.0;
      for (size_t h = 32; h >= 1; h /= 2)
        for (size_t i = 0; i < h; i++) group[i] = group[i] + group[i + h];
      sums.push_back(group[0]);
    }
    v = sums;
    if (v.size() == 1) return v[0];
  }
}

struct Evaluation
{
  double sums[28];
  int32_t num_used = 0, num_outside = 0, num_rejected = 0;
};

static Evaluation Evaluate(const DenseGrid& grid, const std::vector<float>& points, const double* m,
                           const CloudAlignmentOptions& options, const double pivot[3])
{
  const size_t n = points.size() / 3;
  std::vector<std::vector<double>> terms(28, std::vector<double>(n, 0.0));
  Evaluation ev;
  for (size_t i = 0; i < n; i++)
  {
    const double x = static_cast<double>(points[3 * i]), y = static_cast<double>(points[3 * i + 1]),
                 z = static_cast<double>(points[3 * i + 2]);
    if (!(std::isfinite(x) && std::isfinite(y) && std::isfinite(z))) continue;
    double w[3], d = 0.0, g[3];
    for (int r = 0; r < 3; r++) w[r] = ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r];
    if (!EstimateWithGradient(grid, w, d, g))
    {
      ev.num_outside++;
      continue;
    }
    const double r = d - options.target_distance;
    if (!(std::isfinite(r) && std::isfinite(g[0]) && std::isfinite(g[1]) && std::isfinite(g[2]) &&
          std::fabs(r) <= options.max_residual))
    {
      ev.num_rejected++;
      continue;
    }
    ev.num_used++;
    const double q[3] = {w[0] - pivot[0], w[1] - pivot[1], w[2] - pivot[2]};
    const double J[6] = {g[0], g[1], g[2], q[1] * g[2] - q[2] * g[1], q[2] * g[0] - q[0] * g[2],
                         q[0] * g[1] - q[1] * g[0]};
    size_t t = 0;
    for (int j = 0; j < 6; j++)
      for (int k = j; k < 6; k++) terms[t++][i] = J[j] * J[k];
    for (int j = 0; j < 6; j++) terms[21 + static_cast<size_t>(j)][i] = J[j] * r;
    terms[27][i] = r * r;
  }
  for (size_t t = 0; t < 28; t++) ev.sums[t] = TreeSum(terms[t]);
  return ev;
}

// false: degenerate
static bool Solve(const double sums[28], double damping, double delta[6])
{
  double A[6][6], L[6][6] = {}, D[6];
  size_t t = 0;
  for (int j = 0; j < 6; j++)
    for (int k = j; k < 6; k++) A[j][k] = A[k][j] = sums[t++];
  const double scale = 1.0 + damping;
  for (int j = 0; j < 6; j++) A[j][j] = A[j][j] * scale;
  bool degenerate = false;
  for (int j = 0; j < 6; j++)
  {
    double d = A[j][j];
    for (int k = 0; k < j; k++) d = d - (L[j][k] * L[j][k]) * D[k];
    D[j] = d;
    if (!(d > 0.0)) degenerate = true;
    for (int i = j + 1; i < 6; i++)
    {
      double l = A[i][j];
      for (int k = 0; k < j; k++) l = l - (L[i][k] * L[j][k]) * D[k];
      L[i][j] = l / d;
    }
  }
  double y[6], x[6];
  for (int i = 0; i < 6; i++)
  {
    double v = sums[21 + i];
    for (int k = 0; k < i; k++) v = v - L[i][k] * y[k];
    y[i] = v;
  }
  for (int i = 5; i >= 0; i--)
  {
    double v = y[i] / D[i];
    for (int k = i + 1; k < 6; k++) v = v - L[k][i] * x[k];
    x[i] = v;
  }
  for (int i = 0; i < 6; i++)
  {
    delta[i] = -x[i];
    if (!std::isfinite(delta[i])) degenerate = true;
  }
  return !degenerate;
}

static void Update(double m[16], const double delta[6], const double pivot[3])
{
  const double ax = delta[3] * 0.5, ay = delta[4] * 0.5, az = delta[5] * 0.5;
  const double s = 1.0 + ((ax * ax + ay * ay) + az * az);
  const double f = 2.0 / s;
  const double D[3][3] = {{1.0 - f * (ay * ay + az * az), f * (ax * ay - az), f * (ax * az + ay)},
                          {f * (ax * ay + az), 1.0 - f * (ax * ax + az * az), f * (ay * az - ax)},
                          {f * (ax * az - ay), f * (ay * az + ax), 1.0 - f * (ax * ax + ay * ay)}};
  double next[12];
  for (int c = 0; c < 3; c++)
    for (int r = 0; r < 3; r++) next[c * 3 + r] = (D[r][0] * m[4 * c] + D[r][1] * m[4 * c + 1]) + D[r][2] * m[4 * c + 2];
  const double u[3] = {m[12] - pivot[0], m[13] - pivot[1], m[14] - pivot[2]};
  for (int r = 0; r < 3; r++) next[9 + r] = (((D[r][0] * u[0] + D[r][1] * u[1]) + D[r][2] * u[2]) + pivot[r]) + delta[r];
  for (int c = 0; c < 4; c++)
    for (int r = 0; r < 3; r++) m[4 * c + r] = next[c * 3 + r];
}

static CloudAlignment Align(const SignedDistanceField& sdf, const std::vector<float>& points,
                            const std::vector<Isometry3>& poses, const CloudAlignmentOptions& options,
                            const double pivot[3])
{
  CloudAlignment out;
  for (const Isometry3& start : poses)
  {
    Isometry3 pose = start;
    double last_step[6] = {0, 0, 0, 0, 0, 0};
    int32_t steps = 0, evaluations = 0;
    bool last = false;
    uint8_t status;
    Evaluation ev;
    while (true)
    {
      ev = Evaluate(sdf.grid, points, pose.m.data(), options, pivot);
      evaluations++;
      if (ev.num_used < options.min_points)
      {
        status = VGT_HIP_ALIGN_TOO_FEW;
        break;
      }
      if (last)
      {
        status = VGT_HIP_ALIGN_CONVERGED;
        break;
      }
      if (steps >= options.max_iterations)
      {
        status = VGT_HIP_ALIGN_ITERATION_LIMIT;
        break;
      }
      double delta[6];
      if (!Solve(ev.sums, options.damping, delta))
      {
        status = VGT_HIP_ALIGN_DEGENERATE;
        break;
      }
      Update(pose.m.data(), delta, pivot);
      for (int r = 0; r < 6; r++) last_step[r] = delta[r];
      steps++;
      const double v = std::fmax(std::fmax(std::fabs(delta[0]), std::fabs(delta[1])), std::fabs(delta[2]));
      const double w = std::fmax(std::fmax(std::fabs(delta[3]), std::fabs(delta[4])), std::fabs(delta[5]));
      last = v <= options.translation_tolerance && w <= options.rotation_tolerance;
    }
    out.poses.push_back(pose);
    out.status.push_back(status);
    out.num_used.push_back(ev.num_used);
    out.num_outside.push_back(ev.num_outside);
    out.num_rejected.push_back(ev.num_rejected);
    out.sum_squared.push_back(ev.sums[27]);
    out.evaluations.push_back(evaluations);
    out.normal_equations.insert(out.normal_equations.end(), ev.sums, ev.sums + 27);
    out.last_step.insert(out.last_step.end(), last_step, last_step + 6);
  }
  return out;
}
}  // namespace restated

// 4 x 4 x 4 at resolution 1, the value of a cell its x index: the estimate at x is x - 1 everywhere in the grid (cell 0
// holds -0.5 after the half-cell correction, cell i > 0 holds i - 0.5), the gradient (1, 0, 0)
static SignedDistanceField Ramp(const Isometry3& origin)
{
  SignedDistanceField sdf;
  sdf.grid = DenseGrid(origin, "f", 1.0, 4, 4, 4, 0.0f);
  for (int64_t x = 0; x < 4; x++)
    for (int64_t y = 0; y < 4; y++)
      for (int64_t z = 0; z < 4; z++) sdf.grid.SetIndex(x, y, z, static_cast<float>(x));
  return sdf;
}

static std::vector<float> EightPoints()
{
  std::vector<float> points;
  for (int i = 0; i < 8; i++)
  {
    points.push_back(1.25f + 0.25f * static_cast<float>(i));
    points.push_back(0.5f + 0.375f * static_cast<float>(i % 4));
    points.push_back(3.5f - 0.25f * static_cast<float>(i));
  }
  return points;
}

static int RunNoDevice()
{
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double zero[3] = {0.0, 0.0, 0.0};
  const SignedDistanceField sdf = Ramp(Isometry3::Identity());

  // the restatement against answers derived by hand
  {
    // the tree: 1e16 and -1e16 meet at h = 2, before the 1 joins them; left to right the 1 would be lost
    CHECK(restated::TreeSum({1e16, 1.0, -1e16}) == 1.0);
    CHECK(restated::TreeSum(std::vector<double>(65, 1.0)) == 65.0 && restated::TreeSum({-0.0}) == 0.0);
    CHECK(std::signbit(restated::TreeSum(std::vector<double>(64, -0.0))));
    CHECK(!std::signbit(restated::TreeSum(std::vector<double>(63, -0.0))));
    // one point at (2, 1.5, 1.5): d = 1, g = (1, 0, 0), J = (1, 0, 0, 0, 1.5, -1.5) about the origin
    CloudAlignmentOptions options;
    const restated::Evaluation one =
        restated::Evaluate(sdf.grid, {2.0f, 1.5f, 1.5f}, Isometry3::Identity().m.data(), options, zero);
    CHECK(one.num_used == 1 && one.num_outside == 0 && one.num_rejected == 0);
    CHECK(one.sums[0] == 1.0 && one.sums[4] == 1.5 && one.sums[5] == -1.5 && one.sums[1] == 0.0);
    CHECK(one.sums[18] == 2.25 && one.sums[19] == -2.25 && one.sums[20] == 2.25);          // H44, H45, H55
    CHECK(one.sums[21] == 1.0 && one.sums[25] == 1.5 && one.sums[26] == -1.5 && one.sums[27] == 1.0);
    // about the point itself the rotations do nothing; with a target of 1 the residual is 0
    const double at_point[3] = {2.0, 1.5, 1.5};
    options.target_distance = 1.0;
    const restated::Evaluation centred =
        restated::Evaluate(sdf.grid, {2.0f, 1.5f, 1.5f}, Isometry3::Identity().m.data(), options, at_point);
    CHECK(centred.sums[0] == 1.0 && centred.sums[18] == 0.0 && centred.sums[20] == 0.0 && centred.sums[27] == 0.0);
    // outside, beyond max_residual, not finite: counted apart, nothing summed
    options.max_residual = 0.5;
    const restated::Evaluation odd = restated::Evaluate(
        sdf.grid, {2.0f, 1.5f, 1.5f, 3.0f, 1.5f, 1.5f, -1.0f, 1.5f, 1.5f, static_cast<float>(nan), 0.0f, 0.0f},
        Isometry3::Identity().m.data(), options, zero);
    CHECK(odd.num_used == 1 && odd.num_rejected == 1 && odd.num_outside == 1 && odd.sums[27] == 0.0);
    // the solve: a diagonal system, undamped and damped by 1 (the diagonal doubles); a zero pivot
    double sums[28] = {}, delta[6];
    const size_t diagonal[6] = {0, 6, 11, 15, 18, 20};
    for (size_t j = 0; j < 6; j++)
    {
      sums[diagonal[j]] = 2.0;
      sums[21 + j] = 2.0 * static_cast<double>(j + 1);
    }
    CHECK(restated::Solve(sums, 0.0, delta) && delta[0] == -1.0 && delta[3] == -4.0 && delta[5] == -6.0);
    CHECK(restated::Solve(sums, 1.0, delta) && delta[0] == -0.5 && delta[5] == -3.0);
    sums[1] = 1.0;  // H01: x0 = (b0 - H01 x1) / H00 with x1 = b1 / (H11 - H01^2 / H00)
    CHECK(restated::Solve(sums, 0.0, delta) && delta[1] == -(4.0 - 0.5 * 2.0) / 1.5 && delta[0] == -(1.0 + 0.5 * delta[1]));
    sums[1] = 0.0;
    sums[11] = 0.0;
    CHECK(!restated::Solve(sums, 1.0, delta));
    // the update: omega = (0, 0, 2) is a quarter turn about z, exactly; about (1, 0, 0), then v = (0, 0, 0.5)
    Isometry3 pose = Isometry3::Identity();
    pose.m[3] = 7.0;  // (the row nobody reads stays)
    const double step[6] = {0.0, 0.0, 0.5, 0.0, 0.0, 2.0}, about[3] = {1.0, 0.0, 0.0};
    restated::Update(pose.m.data(), step, about);
    CHECK(pose(0, 0) == 0.0 && pose(1, 0) == 1.0 && pose(0, 1) == -1.0 && pose(1, 1) == 0.0 && pose(2, 2) == 1.0);
    CHECK(pose(0, 3) == 1.0 && pose(1, 3) == -1.0 && pose(2, 3) == 0.5 && pose.m[3] == 7.0 && pose.m[15] == 1.0);
    // the loop on the ramp: a flat wall is degenerate and the pose comes back; a cloud sent away has too few points;
    // without a step to take the status is the iteration limit
    CloudAlignmentOptions loop;
    const std::vector<Isometry3> start = {Isometry3::Translation(0.25, 0.0, 0.0), Isometry3::Translation(9.0, 0.0, 0.0)};
    const CloudAlignment got = restated::Align(sdf, EightPoints(), start, loop, zero);
    CHECK(got.status == (std::vector<uint8_t>{VGT_HIP_ALIGN_DEGENERATE, VGT_HIP_ALIGN_TOO_FEW}));
    CHECK(got.evaluations == (std::vector<int32_t>{1, 1}) && got.num_used == (std::vector<int32_t>{8, 0}));
    CHECK(got.num_outside == (std::vector<int32_t>{0, 8}) && got.poses[0].m == start[0].m && got.poses[1].m == start[1].m);
    CHECK(got.last_step == std::vector<double>(12, 0.0));
    loop.max_iterations = 0;
    CHECK(restated::Align(sdf, EightPoints(), start, loop, zero).status ==
          (std::vector<uint8_t>{VGT_HIP_ALIGN_ITERATION_LIMIT, VGT_HIP_ALIGN_TOO_FEW}));
  }

  // argument errors of the layer, raised before a device is asked for
  const std::vector<Isometry3> poses = {Isometry3::Identity()};
  const std::vector<float> points = EightPoints();
  CHECK(ThrowsInvalidArgument([&] { AlignPointCloud(SignedDistanceField(), points, poses); }, "initialized"));
  CHECK(ThrowsInvalidArgument([&] { AlignPointCloud(sdf, std::vector<float>(7, 0.0f), poses); }, "three floats"));
  CHECK(ThrowsInvalidArgument([&] { AlignPointCloud(sdf, std::vector<float>(), poses); }, "not empty"));
  CHECK(ThrowsInvalidArgument([&] { AlignPointCloud(sdf, points, std::vector<Isometry3>()); }, "not empty"));
  {
    auto refused = [&](const char* needle, void (*change)(CloudAlignmentOptions&)) {
      CloudAlignmentOptions options;
      change(options);
      return ThrowsInvalidArgument([&] { AlignPointCloud(sdf, points, poses, options); }, needle);
    };
    CHECK(refused("max_iterations", [](CloudAlignmentOptions& o) { o.max_iterations = -1; }));
    CHECK(refused("min_points", [](CloudAlignmentOptions& o) { o.min_points = 5; }));
    CHECK(refused("damping", [](CloudAlignmentOptions& o) { o.damping = -0.5; }));
    CHECK(refused("max_residual", [](CloudAlignmentOptions& o) { o.max_residual = 0.0; }));
    CHECK(refused("target_distance", [](CloudAlignmentOptions& o) { o.target_distance = std::nan(""); }));
    CHECK(refused("tolerances", [](CloudAlignmentOptions& o) { o.rotation_tolerance = -1.0; }));
    CHECK(refused("three doubles", [](CloudAlignmentOptions& o) { o.pivot = {1.0, 2.0}; }));
    CHECK(refused("finite", [](CloudAlignmentOptions& o) { o.pivot = {1.0, std::nan(""), 0.0}; }));
  }

  // the C ABI's own errors, before the context is looked at
  {
    uint8_t status[1] = {9};
    const float field[64] = {};
    vgt_hip_ctx* stand_in = reinterpret_cast<vgt_hip_ctx*>(&status);
    auto call = [&](vgt_hip_ctx* ctx, int64_t nx, int64_t n, int32_t least, double most, uint8_t* st) {
      return vgt_hip_align_points(ctx, field, nx, 4, 4, 1.0, nullptr, nullptr, points.data(), n, poses[0].m.data(), 1,
                                  nullptr, 3, least, 0.0, most, 0.0, 0.0, 0.0, nullptr, st, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, nullptr);
    };
    CHECK(call(nullptr, 4, 8, 6, 1.0, status) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "null") != nullptr);
    CHECK(call(stand_in, 4, 8, 6, 1.0, nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "null") != nullptr);
    CHECK(call(stand_in, -4, 8, 6, 1.0, status) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "negative") != nullptr);
    CHECK(call(stand_in, 4, 0, 6, 1.0, status) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "not empty") != nullptr);
    CHECK(call(stand_in, int64_t{1} << 31, 8, 6, 1.0, status) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "2^31") != nullptr);
    CHECK(call(stand_in, 4, 8, 5, 1.0, status) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "min_points") != nullptr);
    CHECK(call(stand_in, 4, 8, 6, nan, status) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "max_residual") != nullptr);
    CHECK(status[0] == 9);
    CHECK(vgt_hip_align_points_workspace_bytes(8, 1) == 256 * 5 && vgt_hip_align_points_workspace_bytes(0, 1) == 0);
  }
  return g_failures;
}

template <typename T>
static bool SameBytes(const std::vector<T>& a, const std::vector<T>& b)
{
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// doubles: the same bits, or NaN in both
static bool SameDoubles(const double* a, const double* b, size_t count)
{
  for (size_t i = 0; i < count; i++)
    if (!(std::isnan(a[i]) && std::isnan(b[i])) && std::memcmp(&a[i], &b[i], sizeof(double)) != 0) return false;
  return true;
}

static void CheckAgainstRestatement(const SignedDistanceField& sdf, const std::vector<float>& points,
                                    const std::vector<Isometry3>& poses, const CloudAlignmentOptions& options,
                                    const double pivot[3], const char* what)
{
  const CloudAlignment got = AlignPointCloud(sdf, points, poses, options);
  const CloudAlignment want = restated::Align(sdf, points, poses, options, pivot);
  int counts[4] = {0, 0, 0, 0};
  for (const uint8_t s : want.status) counts[s & 3]++;
  std::printf("%s: converged %d, iteration limit %d, degenerate %d, too few %d\n", what, counts[0], counts[1], counts[2],
              counts[3]);
  CHECK(SameBytes(got.status, want.status) && SameBytes(got.evaluations, want.evaluations));
  CHECK(SameBytes(got.num_used, want.num_used) && SameBytes(got.num_outside, want.num_outside));
  CHECK(SameBytes(got.num_rejected, want.num_rejected));
  CHECK(got.poses.size() == want.poses.size());
  for (size_t i = 0; i < got.poses.size() && i < want.poses.size(); i++)
    CHECK(SameDoubles(got.poses[i].m.data(), want.poses[i].m.data(), 16));
  CHECK(got.sum_squared.size() == want.sum_squared.size() &&
        SameDoubles(got.sum_squared.data(), want.sum_squared.data(), want.sum_squared.size()));
  CHECK(got.normal_equations.size() == want.normal_equations.size() &&
        SameDoubles(got.normal_equations.data(), want.normal_equations.data(), want.normal_equations.size()));
  CHECK(got.last_step.size() == want.last_step.size() &&
        SameDoubles(got.last_step.data(), want.last_step.data(), want.last_step.size()));
}

// a wrapper over packed floats, for the overload that takes a cloud
class PackedCloud : public PointCloudWrapper
{
public:
  explicit PackedCloud(const std::vector<float>& points) : points_(points) {}
  double MaxRange() const override { return 10.0; }
  int64_t Size() const override { return static_cast<int64_t>(points_.size() / 3); }
  const Isometry3& PointCloudOriginTransform() const override { return origin_; }

private:
  void CopyPointLocationIntoFloatPtrImpl(int64_t point_index, float* destination) const override
  {
    for (int r = 0; r < 3; r++) destination[r] = points_[static_cast<size_t>(3 * point_index + r)];
  }
  std::vector<float> points_;
  Isometry3 origin_;
};

static int RunDevice()
{
  // the hand-derived scene: degenerate and too few, the poses back as they came
  {
    const SignedDistanceField sdf = Ramp(Isometry3::Identity());
    const std::vector<Isometry3> start = {Isometry3::Translation(0.25, 0.0, 0.0), Isometry3::Translation(9.0, 0.0, 0.0)};
    const CloudAlignment got = AlignPointCloud(sdf, EightPoints(), start);
    CHECK(got.status == (std::vector<uint8_t>{VGT_HIP_ALIGN_DEGENERATE, VGT_HIP_ALIGN_TOO_FEW}));
    CHECK(got.poses.size() == 2 && got.poses[0].m == start[0].m && got.poses[1].m == start[1].m);
    CHECK(got.num_used == (std::vector<int32_t>{8, 0}) && got.evaluations == (std::vector<int32_t>{1, 1}));
  }
  // a bowl (the distance to a sphere's surface) under an origin transform; 700 points near the surface seen from a
  // sensor frame; 9 hypotheses around the truth, one far away
  {
    const Isometry3 origin = Isometry3::FromQuaternion(std::cos(0.2), 0.0, 0.0, std::sin(0.2), 0.3, -0.2, 0.1);
    SignedDistanceField sdf;
    sdf.grid = DenseGrid(origin, "f", 0.125, 21, 19, 23, 0.0f);
    const double centre[3] = {1.3, 1.1, 1.5}, radius[3] = {0.8, 0.6, 0.7};  // an ellipsoid, so that rotations show
    for (int64_t x = 0; x < 21; x++)
      for (int64_t y = 0; y < 19; y++)
        for (int64_t z = 0; z < 23; z++)
        {
          const double p[3] = {(static_cast<double>(x) + 0.5) * 0.125, (static_cast<double>(y) + 0.5) * 0.125,
                               (static_cast<double>(z) + 0.5) * 0.125};
          double level = 0.0;
          for (int r = 0; r < 3; r++) level += (p[r] - centre[r]) * (p[r] - centre[r]) / (radius[r] * radius[r]);
          sdf.grid.SetIndex(x, y, z, static_cast<float>((std::sqrt(level) - 1.0) * 0.65));
        }
    sdf.grid.SetIndex(5, 4, 6, std::numeric_limits<float>::quiet_NaN());
    uint64_t state = 12345;
    auto next = [&]() {  // uniform in [0, 1)
      state = state * 6364136223846793005ull + 1442695040888963407ull;
      return static_cast<double>(state >> 11) * (1.0 / 9007199254740992.0);
    };
    const Isometry3 truth =
        origin * Isometry3::FromQuaternion(std::cos(0.3), std::sin(0.3) * 0.6, 0.0, std::sin(0.3) * 0.8, 0.2, 0.1, -0.3);
    const Isometry3 sensor_from_world = truth.Inverse();
    std::vector<float> points;
    for (int i = 0; i < 700; i++)
    {
      const double u = next() * 2.0 - 1.0, phi = next() * 6.283185307179586, s = std::sqrt(1.0 - u * u);
      const double in_grid[3] = {centre[0] + radius[0] * s * std::cos(phi), centre[1] + radius[1] * s * std::sin(phi),
                                 centre[2] + radius[2] * u};
      double world[3], local[3];
      for (int r = 0; r < 3; r++)
        world[r] = origin(r, 0) * in_grid[0] + origin(r, 1) * in_grid[1] + origin(r, 2) * in_grid[2] + origin(r, 3);
      for (int r = 0; r < 3; r++)
        local[r] = sensor_from_world(r, 0) * world[0] + sensor_from_world(r, 1) * world[1] +
                   sensor_from_world(r, 2) * world[2] + sensor_from_world(r, 3);
      for (int r = 0; r < 3; r++) points.push_back(static_cast<float>(local[r]));
    }
    points[3 * 11] = std::numeric_limits<float>::quiet_NaN();
    points[3 * 17 + 1] = std::numeric_limits<float>::infinity();
    points[3 * 29 + 2] = 40.0f;  // outside the grid
    std::vector<Isometry3> poses;
    for (int b = 0; b < 9; b++)
    {
      const double angle = 0.01 * b;
      poses.push_back(Isometry3::FromQuaternion(std::cos(angle), std::sin(angle), 0.0, 0.0, 0.02 * b, -0.01 * b, 0.015 * b) *
                      truth);
    }
    poses.push_back(Isometry3::Translation(30.0, 0.0, 0.0) * truth);
    CloudAlignmentOptions options;
    options.max_iterations = 6;
    options.damping = 1e-3;
    options.max_residual = 0.3;
    options.translation_tolerance = 1e-4;
    options.rotation_tolerance = 1e-4;
    const double grid_centre[3] = {0.5 * 21 * 0.125, 0.5 * 19 * 0.125, 0.5 * 23 * 0.125};
    double pivot[3];
    for (int r = 0; r < 3; r++)
      pivot[r] = ((origin(r, 0) * grid_centre[0] + origin(r, 1) * grid_centre[1]) + origin(r, 2) * grid_centre[2]) +
                 origin(r, 3);
    CheckAgainstRestatement(sdf, points, poses, options, pivot, "ellipsoid, the grid's centre as pivot");
    options.pivot = {0.1, -0.2, 0.3};
    options.max_iterations = 2;
    const double given[3] = {0.1, -0.2, 0.3};
    CheckAgainstRestatement(sdf, points, poses, options, given, "ellipsoid, a given pivot, two steps");
    options.max_iterations = 0;
    CheckAgainstRestatement(sdf, points, poses, options, given, "ellipsoid, scored only");
    // the overload that takes a cloud gives the same
    const CloudAlignment packed = AlignPointCloud(sdf, PackedCloud(points), poses, options);
    const CloudAlignment plain = AlignPointCloud(sdf, points, poses, options);
    CHECK(SameBytes(packed.status, plain.status) && SameBytes(packed.num_used, plain.num_used));
    CHECK(SameDoubles(packed.sum_squared.data(), plain.sum_squared.data(), plain.sum_squared.size()));
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
