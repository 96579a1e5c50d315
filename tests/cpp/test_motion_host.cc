// CheckMotions of the C++ host layer (include/vgt_hip/motion_queries.hpp).  --no-device: the restatement in this file
// (interpolation and the reduction per motion, over per-sample values) against answers derived by hand on a two-link
// tree, and the argument errors.  With a device: CheckMotions against that restatement over the per-sample values of
// CheckSphereModel from joint values, bit for bit, with and without the stop flag; then all of it once more with the
// grid on a turned and shifted origin and the tree's base on that origin, against the identity grid's run.
//
// The hand-made scene (tests/test_motion_ref.py has the same one).  Field: 8 x 4 x 4 cells of resolution 1,
// sdf[x][y][z] = x + 1.5: the estimate at a point p with 0.5 <= p_x <= 7.5 is p_x + 0.5.  Tree: link 0 prismatic along x
// at (0, 1.5, 1.5), link 1 fixed on it at (1, 0, 0).  Sphere 0 on link 1, radius 0.25; sphere 1 on link 0, radius 0:
// clearance q + 0.5, always the worst.
#include <vgt_hip.h>
#include <vgt_hip/motion_queries.hpp>

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

template <class Fn>
static bool ThrowsInvalidArgument(const Fn& fn, const char* needle = nullptr)
{
  try
  {
    fn();
  }
  catch (const std::invalid_argument& e)
  {
    if (needle && !std::strstr(e.what(), needle)) std::printf("  message: %s\n", e.what());
    return !needle || std::strstr(e.what(), needle) != nullptr;
  }
  catch (...)
  {
    return false;
  }
  return false;
}

namespace restated
{
const double kNaN = std::numeric_limits<double>::quiet_NaN();

// what the per-sample call returns for one sample
struct Sample
{
  uint8_t status;
  double min_clearance;
  int32_t min_sphere;
  double min_gradient[3];
  uint8_t fk_status;
};

// the joint values of the samples of motion (a, b, n), J doubles per sample
static std::vector<double> Interpolate(const double* a, const double* b, size_t joints, int32_t n)
{
  std::vector<double> q;
  for (int32_t k = 0; k <= n; k++)
    for (size_t j = 0; j < joints; j++)
    {
      if (k == 0)
        q.push_back(a[j]);
      else if (k == n)
        q.push_back(b[j]);
      else
      {
        const double t = static_cast<double>(k) / static_cast<double>(n);
        const double d = b[j] - a[j];
        const double td = t * d;
        q.push_back(a[j] + td);
      }
    }
  return q;
}

static MotionCheck Reduce(const std::vector<Sample>& samples, bool stop_at_collision)
{
  MotionCheck out;
  size_t considered = samples.size();
  for (size_t k = 0; k < samples.size(); k++)
    if (samples[k].status == VGT_HIP_SPHERES_COLLISION)
    {
      out.first_collision = static_cast<int32_t>(k);
      if (stop_at_collision) considered = k + 1;
      break;
    }
  bool no_value = false;
  out.min_clearance = kNaN;
  out.min_gradient = {{kNaN, kNaN, kNaN}};
  for (size_t k = 0; k < considered; k++)
  {
    const Sample& sample = samples[k];
    no_value = no_value || sample.status == VGT_HIP_SPHERES_NO_VALUE;
    out.fk_status |= sample.fk_status;
    if (!std::isnan(sample.min_clearance) && (out.min_sample < 0 || sample.min_clearance < out.min_clearance))
    {
      out.min_clearance = sample.min_clearance;
      out.min_sample = static_cast<int32_t>(k);
      out.min_sphere = sample.min_sphere;
      out.min_gradient = {{sample.min_gradient[0], sample.min_gradient[1], sample.min_gradient[2]}};
    }
  }
  out.status = out.first_collision >= 0 ? VGT_HIP_MOTION_COLLISION : no_value ? VGT_HIP_MOTION_NO_VALUE : VGT_HIP_MOTION_CLEAR;
  return out;
}

// The hand-made scene's sample at joint value q, by the formulas at the head of this file (q a multiple of 0.5).
static Sample HandSample(double q, double minimum_clearance, bool outside_is_collision, const double* limits)
{
  Sample sample{VGT_HIP_SPHERES_NO_VALUE, kNaN, -1, {kNaN, kNaN, kNaN}, 0};
  if (limits && (q < limits[0] || q > limits[1])) sample.fk_status |= VGT_HIP_FK_OUTSIDE_LIMITS;
  if (!std::isfinite(q))
  {
    sample.fk_status |= VGT_HIP_FK_NOT_COMPUTABLE;
    if (outside_is_collision) sample.status = VGT_HIP_SPHERES_COLLISION;
    return sample;
  }
  const bool has0 = q + 1.0 >= 0.0 && q + 1.0 < 8.0, has1 = q >= 0.0 && q < 8.0;  // sphere 0 on link 1, sphere 1 on link 0
  const double c0 = q + 1.25, c1 = q + 0.5;
  const int outside = (has0 ? 0 : 1) + (has1 ? 0 : 1);
  const int below = (has0 && c0 <= minimum_clearance ? 1 : 0) + (has1 && c1 <= minimum_clearance ? 1 : 0);
  if (has1 || has0)
  {
    sample.min_sphere = has1 ? 1 : 0;
    sample.min_clearance = has1 ? c1 : c0;
    sample.min_gradient[0] = 1.0;
    sample.min_gradient[1] = sample.min_gradient[2] = 0.0;
  }
  if (below > 0 || (outside_is_collision && outside > 0))
    sample.status = VGT_HIP_SPHERES_COLLISION;
  else if (sample.min_sphere >= 0)
    sample.status = VGT_HIP_SPHERES_CLEAR;
  return sample;
}

static MotionCheck HandMotion(double a, double b, int32_t n, const MotionOptions& options)
{
  std::vector<Sample> samples;
  for (double q : Interpolate(&a, &b, 1, n))
    samples.push_back(HandSample(q, options.minimum_clearance, options.outside_is_collision,
                                 options.joint_limits.empty() ? nullptr : options.joint_limits.data()));
  return Reduce(samples, options.stop_at_collision);
}
}  // namespace restated

static bool SameDouble(double a, double b)
{
  return (std::isnan(a) && std::isnan(b)) || std::memcmp(&a, &b, sizeof(double)) == 0;
}

static bool Same(const MotionCheck& a, const MotionCheck& b)
{
  return a.status == b.status && a.first_collision == b.first_collision && SameDouble(a.min_clearance, b.min_clearance) &&
         a.min_sample == b.min_sample && a.min_sphere == b.min_sphere && SameDouble(a.min_gradient[0], b.min_gradient[0]) &&
         SameDouble(a.min_gradient[1], b.min_gradient[1]) && SameDouble(a.min_gradient[2], b.min_gradient[2]) &&
         a.fk_status == b.fk_status;
}

static KinematicTree TwoLinks()
{
  KinematicLink slide, tool;
  slide.parent = -1;
  slide.joint_type = VGT_HIP_JOINT_PRISMATIC;
  slide.joint_index = 0;
  slide.axis = {{1.0, 0.0, 0.0}};
  slide.origin = Isometry3::Translation(0.0, 1.5, 1.5);
  tool.parent = 0;
  tool.joint_type = VGT_HIP_JOINT_FIXED;
  tool.origin = Isometry3::Translation(1.0, 0.0, 0.0);
  return KinematicTree({slide, tool}, 1);
}

static SphereModel TwoSpheres()
{
  SphereModel model;
  model.link = {1, 0};
  model.xyzr = {{{0.0, 0.0, 0.0, 0.25}}, {{0.0, 0.0, 0.0, 0.0}}};
  return model;
}

// A grid origin turned by 0.7 about (0.3, -0.5, 0.8) -- an axis that is none of x, y, z: no entry of the rotation is near
// 0 or +-1 -- and shifted.
static Isometry3 TurnedOrigin()
{
  const double s = std::sin(0.35) / std::sqrt(0.3 * 0.3 + 0.5 * 0.5 + 0.8 * 0.8);
  return Isometry3::FromQuaternion(std::cos(0.35), 0.3 * s, -0.5 * s, 0.8 * s, 0.4, -0.2, 0.05);
}

static SignedDistanceField Ramp(const Isometry3& origin = Isometry3::Identity())
{
  SignedDistanceField sdf;
  sdf.grid = DenseGrid(origin, "f", 1.0, 8, 4, 4, 0.0f);
  for (int64_t x = 0; x < 8; x++)
    for (int64_t y = 0; y < 4; y++)
      for (int64_t z = 0; z < 4; z++) sdf.grid.SetIndex(x, y, z, static_cast<float>(x) + 1.5f);
  return sdf;
}

static int RunNoDevice()
{
  using restated::HandMotion;
  const double nan = restated::kNaN, inf = std::numeric_limits<double>::infinity();
  // the interpolation keeps the endpoints' bits and does not read joint_to without steps
  {
    const double a[2] = {0.1, -0.0}, b[2] = {0.7, 5.0};
    const std::vector<double> q = restated::Interpolate(a, b, 2, 3);
    CHECK(q.size() == 8 && std::memcmp(&q[0], a, 16) == 0 && std::memcmp(&q[6], b, 16) == 0);
    CHECK(q[2] == 0.1 + (1.0 / 3.0) * (0.7 - 0.1) && q[5] == -0.0 + (2.0 / 3.0) * (5.0 - -0.0));
    const double none[2] = {nan, nan};
    const std::vector<double> one = restated::Interpolate(a, none, 2, 0);
    CHECK(one.size() == 2 && std::memcmp(&one[0], a, 16) == 0);
  }
  // q = 5, 4, 3, 2, 1: clearances 5.5, 4.5, 3.5, 2.5, 1.5
  {
    MotionOptions options;
    options.minimum_clearance = 3.5;
    MotionCheck got = HandMotion(5.0, 1.0, 4, options);
    CHECK(got.status == VGT_HIP_MOTION_COLLISION && got.first_collision == 2 && got.min_sample == 4 && got.min_sphere == 1);
    CHECK(got.min_clearance == 1.5 && got.min_gradient[0] == 1.0 && got.min_gradient[2] == 0.0 && got.fk_status == 0);
    options.stop_at_collision = true;
    got = HandMotion(5.0, 1.0, 4, options);
    CHECK(got.status == VGT_HIP_MOTION_COLLISION && got.first_collision == 2 && got.min_sample == 2 && got.min_clearance == 3.5);
    options.minimum_clearance = 1.0;
    got = HandMotion(5.0, 1.0, 4, options);
    CHECK(got.status == VGT_HIP_MOTION_CLEAR && got.first_collision == -1 && got.min_sample == 4);
    got = HandMotion(3.0, 3.0, 5, options);  // ties: the lowest sample
    CHECK(got.status == VGT_HIP_MOTION_CLEAR && got.min_sample == 0 && got.min_clearance == 3.5);
  }
  // samples without a value; the limits and a value that cannot be used
  {
    MotionOptions options;
    MotionCheck got = HandMotion(5.0, 20.0, 3, options);
    CHECK(got.status == VGT_HIP_MOTION_NO_VALUE && got.first_collision == -1 && got.min_sample == 0 && got.min_clearance == 5.5);
    options.outside_is_collision = true;
    got = HandMotion(5.0, 20.0, 3, options);
    CHECK(got.status == VGT_HIP_MOTION_COLLISION && got.first_collision == 1);
    options = MotionOptions();
    got = HandMotion(20.0, 30.0, 2, options);
    CHECK(got.status == VGT_HIP_MOTION_NO_VALUE && got.min_sample == -1 && got.min_sphere == -1 && std::isnan(got.min_clearance));
    CHECK(std::isnan(got.min_gradient[0]) && std::isnan(got.min_gradient[1]) && std::isnan(got.min_gradient[2]));
    options.joint_limits = {0.0, 6.0};
    CHECK(HandMotion(5.0, inf, 2, options).fk_status == 3 && HandMotion(5.0, 7.0, 2, options).fk_status == 2);
    CHECK(HandMotion(5.0, 1.0, 0, options).fk_status == 0 && HandMotion(2.0, nan, 0, options).min_clearance == 2.5);
    options.minimum_clearance = 5.5;
    options.stop_at_collision = true;
    got = HandMotion(5.0, 7.0, 2, options);
    CHECK(got.first_collision == 0 && got.fk_status == 0);  // (the later samples do not exist)
  }

  // argument errors of the layer, before a device is asked for
  {
    const KinematicTree tree = TwoLinks();
    const SphereModel model = TwoSpheres();
    const SignedDistanceField sdf = Ramp();
    CHECK(ThrowsInvalidArgument([&] { CheckMotions(SignedDistanceField(), model, tree, {0.0}, {1.0}, {2}); }, "initialized"));
    CHECK(ThrowsInvalidArgument([&] { CheckMotions(sdf, model, tree, {0.0, 1.0}, {1.0}, {2}); }, "one value per motion"));
    CHECK(ThrowsInvalidArgument([&] { CheckMotions(sdf, model, tree, {0.0, 1.0, 2.0}, {1.0, 2.0, 3.0}, {2, 3}); },
                                "one count per motion"));
    CHECK(ThrowsInvalidArgument([&] { CheckMotions(sdf, model, tree, {0.0, 1.0, 2.0}, {1.0, 2.0, 3.0}, {2, 3, -3}); },
                                "motion 2: num_steps -3"));
    CHECK(ThrowsInvalidArgument([&] { CheckMotions(sdf, model, tree, {0.0, 1.0}, {1.0, 2.0}, {-1}); },
                                "motion 0: num_steps -1"));
    SphereModel bad = model;
    bad.link[1] = 2;
    CHECK(ThrowsInvalidArgument([&] { CheckMotions(sdf, bad, tree, {0.0}, {1.0}, {2}); }, "sphere 1: link 2"));
    bad = model;
    bad.xyzr[0][3] = -1.0;
    CHECK(ThrowsInvalidArgument([&] { CheckMotions(sdf, bad, tree, {0.0}, {1.0}, {2}); }, "sphere 0: the radius"));
    bad = model;
    bad.link.push_back(0);
    CHECK(ThrowsInvalidArgument([&] { CheckMotions(sdf, bad, tree, {0.0}, {1.0}, {2}); }, "one link"));
    MotionOptions options;
    options.minimum_clearance = nan;
    CHECK(ThrowsInvalidArgument([&] { CheckMotions(sdf, model, tree, {0.0}, {1.0}, {2}, options); }, "minimum_clearance"));
    options = MotionOptions();
    options.joint_limits = {0.0};
    CHECK(ThrowsInvalidArgument([&] { CheckMotions(sdf, model, tree, {0.0}, {1.0}, {2}, options); }, "joint_limits"));
    std::vector<KinematicLink> many(641);
    for (size_t i = 0; i < many.size(); i++) many[i].parent = static_cast<int32_t>(i) - 1;
    CHECK(ThrowsInvalidArgument([&] { CheckMotions(sdf, SphereModel(), KinematicTree(many, 0), {}, {}, {2}); },
                                "640 links, this one has 641"));
    // nothing to compute: no device is needed
    CHECK(CheckMotions(sdf, model, tree, {}, {}, {}).empty() && CheckMotions(sdf, model, tree, {}, {}, {7}).empty());
  }

  // the C ABI's own errors, before the context or the tree is looked at
  {
    double memory[64] = {};
    vgt_hip_ctx* ctx = reinterpret_cast<vgt_hip_ctx*>(memory);
    const vgt_hip_kinematics* fake = reinterpret_cast<const vgt_hip_kinematics*>(memory);
    const float* field = reinterpret_cast<const float*>(memory);
    const int32_t link[2] = {0, 0};
    const int32_t steps[3] = {1, -3, -4};
    double xyzr[8] = {0, 0, 0, 0.1, 0, 0, 0, 0.1};
    uint8_t status[3] = {9, 9, 9};
    auto call = [&](int64_t motions, const int32_t* num_steps, int32_t uniform, uint32_t flags, double resolution) {
      return vgt_hip_check_motions(ctx, field, 4, 4, 4, resolution, nullptr, nullptr, xyzr, link, 2, fake, memory, memory,
                                   num_steps, uniform, motions, nullptr, nullptr, 0.0, flags, status, nullptr, nullptr,
                                   nullptr, nullptr, nullptr, nullptr);
    };
    CHECK(call(3, steps, 0, 0, 1.0) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "motion 1: num_steps -3") != nullptr);
    CHECK(call(3, nullptr, -2, 0, 1.0) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "uniform_steps -2") != nullptr);
    CHECK(call(3, nullptr, 2, 4, 1.0) == VGT_HIP_ERR_INVALID_ARGUMENT && std::strstr(vgt_hip_last_error(), "flag") != nullptr);
    CHECK(call(3, nullptr, 2, 0, 0.0) == VGT_HIP_ERR_INVALID_ARGUMENT && std::strstr(vgt_hip_last_error(), "resolution") != nullptr);
    CHECK(call(-1, nullptr, 2, 0, 1.0) == VGT_HIP_ERR_INVALID_ARGUMENT && std::strstr(vgt_hip_last_error(), "negative") != nullptr);
    xyzr[7] = nan;
    CHECK(call(1, steps, 0, 0, 1.0) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "sphere 1: the radius") != nullptr);
    xyzr[7] = 0.1;
    CHECK(call(1, steps, 0, 0, 1.0) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "another context") != nullptr);
    CHECK(call(0, steps, 0, 3, 1.0) == VGT_HIP_OK);
    CHECK(status[0] == 9 && status[1] == 9 && status[2] == 9);
    CHECK(vgt_hip_motion_tile_samples(1) >= vgt_hip_motion_tile_samples(640) && vgt_hip_motion_tile_samples(640) == 1);
    CHECK(vgt_hip_motion_tile_samples(641) == 0);
  }
  return g_failures;
}

static int RunDevice()
{
  const KinematicTree tree = TwoLinks();
  const SphereModel model = TwoSpheres();
  const SignedDistanceField sdf = Ramp();
  // motions of the hand-made scene, 70 of them, at multiples of 0.5 so that the formulas are exact; step counts on both
  // sides of the kernel's tile sizes
  std::vector<double> from, to;
  std::vector<int32_t> steps;
  const int32_t counts[10] = {0, 1, 2, 4, 8, 16, 32, 64, 128, 256};  // (powers of two: t and t * (b - a) are exact)
  for (int e = 0; e < 70; e++)
  {
    const int32_t n = counts[e % 10];
    const double a = 0.5 * (e % 13), span = 0.5 * ((e * 7) % 9 - 4);
    from.push_back(a);
    to.push_back(a + span * n);
    steps.push_back(n);
  }
  from[11] = std::numeric_limits<double>::quiet_NaN();
  to[12] = std::numeric_limits<double>::infinity();
  // The second pass: the ramp on the turned and shifted origin and the tree's base on that origin, so that the tree is
  // where it was in the grid.  The comparison with the layer's per-sample call stays bit for bit; the answers by hand
  // give way to the identity grid's run of the same call, which they hold.  There the threshold is off the lattice of
  // the clearances (multiples of 0.25): the rounding of the two more transforms would decide on which side of `<=` a
  // sample with a clearance equal to the threshold lands.
  const Isometry3 origin = TurnedOrigin();
  for (int turned = 0; turned < 2; turned++)
  {
    const SignedDistanceField grid = turned ? Ramp(origin) : sdf;
    int compared = 0, on_an_end_face = 0;
    for (int variant = 0; variant < 4; variant++)
    {
      MotionOptions options;
      options.minimum_clearance = turned ? 2.125 : 2.0;
      options.stop_at_collision = (variant & 1) != 0;
      options.outside_is_collision = (variant & 2) != 0;
      if (variant >= 2) options.joint_limits = {0.0, 6.0};
      const MotionOptions plain_options = options;
      if (turned)
      {
        options.has_world_from_base = true;
        options.world_from_base = origin;
      }
      const std::vector<MotionCheck> got = CheckMotions(grid, model, tree, from, to, steps, options);
      CHECK(got.size() == 70);
      // the same call on the identity grid
      const std::vector<MotionCheck> plain = turned ? CheckMotions(sdf, model, tree, from, to, steps, plain_options) : got;
      CHECK(plain.size() == 70);
      int statuses[3] = {0, 0, 0};
      for (size_t e = 0; e < got.size(); e++)
      {
        // by hand
        const MotionCheck hand = restated::HandMotion(from[e], to[e], steps[e], options);
        if (!turned && !Same(got[e], hand))
        {
          std::printf("  motion %zu variant %d: status %d/%d first %d/%d sample %d/%d clearance %g/%g fk %d/%d\n", e, variant,
                      got[e].status, hand.status, got[e].first_collision, hand.first_collision, got[e].min_sample,
                      hand.min_sample, got[e].min_clearance, hand.min_clearance, got[e].fk_status, hand.fk_status);
          CHECK(false);
        }
        // the per-sample call of the layer, reduced here
        const std::vector<double> q = restated::Interpolate(&from[e], &to[e], 1, steps[e]);
        JointSphereModelOptions sample_options;
        sample_options.minimum_clearance = options.minimum_clearance;
        sample_options.outside_is_collision = options.outside_is_collision;
        sample_options.joint_limits = options.joint_limits;
        sample_options.has_world_from_base = options.has_world_from_base;
        sample_options.world_from_base = options.world_from_base;
        const JointSphereModelChecks flat = CheckSphereModel(grid, model, tree, q, sample_options);
        std::vector<restated::Sample> samples;
        for (size_t k = 0; k < q.size(); k++)
          samples.push_back({flat.checks.status[k], flat.checks.min_clearance[k], flat.checks.min_sphere[k],
                             {flat.checks.min_gradient[3 * k], flat.checks.min_gradient[3 * k + 1],
                              flat.checks.min_gradient[3 * k + 2]},
                             flat.fk_status[k]});
        CHECK(Same(got[e], restated::Reduce(samples, options.stop_at_collision)));
        if (got[e].status < 3) statuses[got[e].status]++;
        if (!turned) continue;
        // A sphere centre on an end face of the grid in x (the spheres are at q + 1 and q) is inside or outside by the
        // rounding of the transforms; every motion without such a sample is the identity grid's, up to that rounding,
        // and its gradient the identity grid's turned by the origin's rotation.
        bool end_face = false;
        for (const double value : q) end_face = end_face || value == -1.0 || value == 0.0 || value == 7.0 || value == 8.0;
        if (end_face)
        {
          on_an_end_face++;
          continue;
        }
        compared++;
        const auto close = [](double a, double b) {
          return (std::isnan(a) && std::isnan(b)) || a == b || std::fabs(a - b) <= 1e-12;
        };
        bool as_plain = got[e].status == plain[e].status && got[e].first_collision == plain[e].first_collision &&
                        got[e].min_sample == plain[e].min_sample && got[e].min_sphere == plain[e].min_sphere &&
                        got[e].fk_status == plain[e].fk_status && close(got[e].min_clearance, plain[e].min_clearance);
        for (int r = 0; r < 3; r++)
        {
          const double* g = plain[e].min_gradient.data();
          as_plain = as_plain && close(got[e].min_gradient[r], (origin(r, 0) * g[0] + origin(r, 1) * g[1]) + origin(r, 2) * g[2]);
        }
        if (!as_plain)
        {
          std::printf("  motion %zu variant %d, turned/identity: status %d/%d first %d/%d sample %d/%d sphere %d/%d clearance %.17g/%.17g fk %d/%d gradient (%g %g %g)/(%g %g %g)\n",
                      e, variant, got[e].status, plain[e].status, got[e].first_collision, plain[e].first_collision,
                      got[e].min_sample, plain[e].min_sample, got[e].min_sphere, plain[e].min_sphere, got[e].min_clearance,
                      plain[e].min_clearance, got[e].fk_status, plain[e].fk_status, got[e].min_gradient[0],
                      got[e].min_gradient[1], got[e].min_gradient[2], plain[e].min_gradient[0], plain[e].min_gradient[1],
                      plain[e].min_gradient[2]);
          CHECK(false);
        }
      }
      CHECK(statuses[0] > 0 && statuses[1] > 0 && (variant >= 2 || statuses[2] > 0));
    }
    // per variant the 31 motions that have a sample with q in {-1, 0, 7, 8}
    if (turned) CHECK(on_an_end_face == 4 * 31 && compared == 4 * (70 - 31));
  }
  // one count for all motions
  {
    const std::vector<MotionCheck> got = CheckMotions(sdf, model, tree, {5.0, 3.0}, {1.0, 3.0}, {4});
    CHECK(got.size() == 2 && got[0].min_sample == 4 && got[0].min_clearance == 1.5 && got[1].min_sample == 0);
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
