// SelfCollisionPairs and CheckSelfCollision of the C++ host layer (include/vgt_hip/self_collision.hpp).  --no-device: the
// pair generator against lists written by hand, the restatement in this file (the pair arithmetic, the order and the
// status, over centres) against answers derived by hand, and the argument errors.  With a device: CheckSelfCollision
// against the hand-made answers and against that restatement over the poses of ComputeLinkPoses, with
// ClearanceJointGradient's summed form for the gradient, bit for bit.
//
// The hand-made scene.  Tree: the links 0 and 1 slide along x on the base, each with a joint of its own (q0, q1); link 2
// is fixed on link 1.  Sphere 0 on link 0, radius 0.25, centre (q0, 0, 0); the spheres 1 and 2 are twins on link 1,
// radius 0.5, centre (q1, 0, 0); sphere 3 on link 2 at (0, 3, 0) of it, radius 0.25, centre (q1, 3, 0).  With joint values
// that are multiples of 0.25: the pairs (0, 1) and (0, 2) tie at |q0 - q1| - 0.75 with direction (sign(q0 - q1), 0, 0) and
// gradient (sign, -sign) -- NaN, NaN where q0 == q1 --; the pair (1, 3) is always 3 - 0.75 = 2.25.
#include <vgt_hip.h>
#include <vgt_hip/self_collision.hpp>

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

struct Configuration
{
  uint8_t status = VGT_HIP_SELF_NO_VALUE;
  int32_t num_below = 0, num_without_value = 0, min_pair = -1;
  double min_clearance = kNaN;
  double direction[3] = {kNaN, kNaN, kNaN};
  std::vector<double> clearance;
};

// one configuration from its spheres' world centres [S][3] and radii
static Configuration Reduce(const std::vector<double>& centres, const std::vector<double>& radii,
                            const std::vector<SpherePair>& pairs, double minimum, bool no_value_is_collision)
{
  Configuration out;
  const int32_t spheres = static_cast<int32_t>(radii.size());
  for (size_t p = 0; p < pairs.size(); p++)
  {
    const int32_t a = pairs[p][0], b = pairs[p][1];
    double clearance = kNaN;
    volatile double e[3] = {kNaN, kNaN, kNaN}, dist = kNaN;
    if (a >= 0 && a < spheres && b >= 0 && b < spheres)
    {
      for (int r = 0; r < 3; r++) e[r] = centres[3 * a + r] - centres[3 * b + r];
      const volatile double s0 = e[0] * e[0], s1 = e[1] * e[1], s2 = e[2] * e[2];
      const volatile double s01 = s0 + s1;
      const volatile double d2 = s01 + s2;
      dist = std::sqrt(d2);
      const volatile double first = dist - radii[a];
      clearance = first - radii[b];
    }
    out.clearance.push_back(clearance);
    if (std::isnan(clearance))
    {
      out.num_without_value++;
      continue;
    }
    if (clearance <= minimum) out.num_below++;
    if (out.min_pair < 0 || clearance < out.min_clearance)
    {
      out.min_pair = static_cast<int32_t>(p);
      out.min_clearance = clearance;
      for (int r = 0; r < 3; r++) out.direction[r] = e[r] / dist;
    }
  }
  if (out.num_below > 0 || (no_value_is_collision && out.num_without_value > 0))
    out.status = VGT_HIP_SELF_COLLISION;
  else if (out.min_pair >= 0)
    out.status = VGT_HIP_SELF_CLEAR;
  return out;
}
}  // namespace restated

static bool SameDouble(double a, double b)
{
  return (std::isnan(a) && std::isnan(b)) || std::memcmp(&a, &b, sizeof(double)) == 0;
}

static KinematicTree ThreeLinks()
{
  KinematicLink first, second, bar;
  first.parent = -1;
  first.joint_type = VGT_HIP_JOINT_PRISMATIC;
  first.joint_index = 0;
  first.axis = {{1.0, 0.0, 0.0}};
  first.origin = Isometry3::Identity();
  second = first;
  second.joint_index = 1;
  bar.parent = 1;
  bar.joint_type = VGT_HIP_JOINT_FIXED;
  bar.origin = Isometry3::Identity();
  return KinematicTree({first, second, bar}, 2);
}

static SphereModel FourSpheres()
{
  SphereModel model;
  model.link = {0, 1, 1, 2};
  model.xyzr = {{{0.0, 0.0, 0.0, 0.25}}, {{0.0, 0.0, 0.0, 0.5}}, {{0.0, 0.0, 0.0, 0.5}}, {{0.0, 3.0, 0.0, 0.25}}};
  return model;
}

static std::vector<double> HandCentres(double q0, double q1)
{
  return {q0, 0.0, 0.0, q1, 0.0, 0.0, q1, 0.0, 0.0, q1, 3.0, 0.0};
}

static int RunNoDevice()
{
  const double nan = restated::kNaN;
  const KinematicTree tree = ThreeLinks();
  const SphereModel model = FourSpheres();
  const std::vector<double> radii = {0.25, 0.5, 0.5, 0.25};
  // the pair generator
  {
    const std::vector<SpherePair> all = SelfCollisionPairs(model, tree);
    CHECK((all == std::vector<SpherePair>{{{0, 1}}, {{0, 2}}, {{0, 3}}, {{1, 3}}, {{2, 3}}}));
    SelfCollisionPairOptions apart;
    apart.skip_adjacent = true;
    CHECK((SelfCollisionPairs(model, tree, {}, apart) == std::vector<SpherePair>{{{0, 1}}, {{0, 2}}, {{0, 3}}}));
    CHECK((SelfCollisionPairs(model, tree, {{{1, 0}}, {{0, 2}}}) == std::vector<SpherePair>{{{1, 3}}, {{2, 3}}}));
    CHECK(SelfCollisionPairs(SphereModel(), tree).empty());
    SphereModel bad = model;
    bad.link[3] = 3;
    CHECK(ThrowsInvalidArgument([&] { SelfCollisionPairs(bad, tree); }, "sphere 3: link 3 is not in [0, num_links)"));
    CHECK(ThrowsInvalidArgument([&] { SelfCollisionPairs(model, tree, {{{0, 1}}, {{5, 1}}}); },
                                "ignored pair 1: link 5 is not in [0, num_links)"));
    bad = model;
    bad.link.pop_back();
    CHECK(ThrowsInvalidArgument([&] { SelfCollisionPairs(bad, tree); }, "one link and one"));
  }
  // the restatement on the hand-made scene
  const std::vector<SpherePair> pairs = {{{1, 3}}, {{0, 1}}, {{0, 2}}, {{0, 7}}};
  {
    restated::Configuration got = restated::Reduce(HandCentres(2.0, 0.5), radii, pairs, 0.75, false);
    CHECK(got.clearance[0] == 2.25 && got.clearance[1] == 0.75 && got.clearance[2] == 0.75 && std::isnan(got.clearance[3]));
    CHECK(got.min_pair == 1 && got.min_clearance == 0.75 && got.num_below == 2 && got.num_without_value == 1);
    CHECK(got.status == VGT_HIP_SELF_COLLISION && got.direction[0] == 1.0 && got.direction[1] == 0.0);
    got = restated::Reduce(HandCentres(-1.0, 0.5), radii, pairs, 0.5, false);
    CHECK(got.status == VGT_HIP_SELF_CLEAR && got.direction[0] == -1.0 && got.min_clearance == 0.75);
    CHECK(restated::Reduce(HandCentres(-1.0, 0.5), radii, pairs, 0.5, true).status == VGT_HIP_SELF_COLLISION);
    got = restated::Reduce(HandCentres(0.5, 0.5), radii, pairs, 0.0, false);
    CHECK(got.min_pair == 1 && got.min_clearance == -0.75 && std::isnan(got.direction[0]) && std::isnan(got.direction[2]));
    got = restated::Reduce(HandCentres(nan, 0.5), radii, pairs, 0.0, false);
    CHECK(got.min_pair == 0 && got.num_without_value == 3 && got.status == VGT_HIP_SELF_CLEAR);
    got = restated::Reduce(HandCentres(nan, nan), radii, pairs, 0.0, false);
    CHECK(got.min_pair == -1 && got.status == VGT_HIP_SELF_NO_VALUE && std::isnan(got.min_clearance));
  }
  // argument errors of the layer, before a device is asked for
  {
    const std::vector<double> q = {0.0, 1.0};
    SelfCollisionOptions options;
    options.minimum_clearance = nan;
    CHECK(ThrowsInvalidArgument([&] { CheckSelfCollision(model, tree, pairs, q, options); }, "must not be NaN"));
    options = SelfCollisionOptions();
    options.joint_limits = {0.0};
    CHECK(ThrowsInvalidArgument([&] { CheckSelfCollision(model, tree, pairs, q, options); }, "joint_limits"));
    CHECK(ThrowsInvalidArgument([&] { CheckSelfCollision(model, tree, pairs, q); }, "pair 3: sphere 7 is outside [0, 4)"));
    CHECK(ThrowsInvalidArgument([&] { CheckSelfCollision(model, tree, {{{0, 1}}, {{2, 2}}}, q); },
                                "pair 1: (2, 2) is not ascending"));
    CHECK(ThrowsInvalidArgument([&] { CheckSelfCollision(model, tree, {{{0, 1}}}, {0.0, 1.0, 2.0}); },
                                "one value per configuration and joint"));
    CHECK(ThrowsInvalidArgument([&] { CheckSelfCollision(model, tree, {{{0, 1}}}, q, {}, 2); },
                                "one value per configuration and joint"));
    SphereModel bad = model;
    bad.link[1] = 3;
    CHECK(ThrowsInvalidArgument([&] { CheckSelfCollision(bad, tree, {{{0, 1}}}, q); }, "sphere 1: link 3 is not in"));
    bad = model;
    bad.xyzr[2][3] = nan;
    CHECK(ThrowsInvalidArgument([&] { CheckSelfCollision(bad, tree, {{{0, 1}}}, q); }, "sphere 2: the radius"));
    bad = model;
    bad.xyzr.resize(2100, {{0.0, 0.0, 0.0, 0.1}});
    bad.link.resize(2100, 0);
    CHECK(ThrowsInvalidArgument([&] { CheckSelfCollision(bad, tree, {{{0, 1}}}, q); },
                                "this model has 3 links and 2100 spheres"));
    // no configurations: no device is needed
    const SelfCollisionChecks none = CheckSelfCollision(model, tree, {{{0, 1}}}, {});
    CHECK(none.status.empty() && none.joint_gradient.empty() && none.fk_status.empty());
    CHECK(vgt_hip_self_collision_tile_samples(1, 0) == 64 && vgt_hip_self_collision_tile_samples(680, 0) == 1 &&
          vgt_hip_self_collision_tile_samples(681, 0) == 0 && vgt_hip_self_collision_tile_samples(1, 2038) == 0);
  }
  // the C ABI's own errors, before the context is looked at
  {
    double memory[64] = {};
    vgt_hip_ctx* stand_in = reinterpret_cast<vgt_hip_ctx*>(memory);
    const vgt_hip_kinematics* handle = reinterpret_cast<const vgt_hip_kinematics*>(memory);
    uint8_t status[2] = {9, 9};
    CHECK(vgt_hip_check_self_collision(stand_in, nullptr, nullptr, 0, nullptr, 0, handle, memory, 2, nullptr, nullptr, nan,
                                       0, status, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "minimum_clearance must not be NaN") != nullptr);
    CHECK(vgt_hip_check_self_collision(stand_in, nullptr, nullptr, 0, nullptr, 0, handle, memory, 2, nullptr, nullptr, 0.0,
                                       2, status, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "unknown self-collision flag") != nullptr);
    CHECK(vgt_hip_check_self_collision_poses(stand_in, nullptr, nullptr, 0, nullptr, 0, memory, 2, 1, nullptr, 0.0, 0,
                                             status, nullptr, nullptr, nullptr, nullptr, nullptr, memory,
                                             nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "the joint gradient needs the kinematic tree") != nullptr);
    CHECK(vgt_hip_check_self_collision(stand_in, nullptr, nullptr, 0, nullptr, 0, handle, nullptr, 0, nullptr, nullptr, 0.0,
                                       0, status, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       nullptr) == VGT_HIP_OK);
    CHECK(status[0] == 9 && status[1] == 9);
  }
  return g_failures;
}

static int RunDevice()
{
  const KinematicTree tree = ThreeLinks();
  const SphereModel model = FourSpheres();
  const std::vector<double> radii = {0.25, 0.5, 0.5, 0.25};
  const std::vector<SpherePair> pairs = {{{1, 3}}, {{0, 1}}, {{0, 2}}, {{0, 3}}};
  // 70 configurations at multiples of 0.25, q0 on both sides of q1 and on it
  std::vector<double> q;
  for (int b = 0; b < 70; b++)
  {
    q.push_back(0.25 * ((b * 7) % 23) - 2.0);
    q.push_back(0.25 * ((b * 5) % 11) - 1.0);
  }
  q[2 * 11] = std::numeric_limits<double>::quiet_NaN();
  q[2 * 12 + 1] = std::numeric_limits<double>::infinity();
  q[2 * 13] = q[2 * 13 + 1] = std::numeric_limits<double>::quiet_NaN();
  for (int variant = 0; variant < 4; variant++)
  {
    SelfCollisionOptions options;
    options.minimum_clearance = (variant & 1) ? 0.25 : 0.0;
    options.no_value_is_collision = variant >= 2;
    options.per_pair = true;
    if (variant >= 2) options.joint_limits = {-1.0, 1.0, -0.5, 2.0};
    const SelfCollisionChecks got = CheckSelfCollision(model, tree, pairs, q, options);
    CHECK(got.status.size() == 70 && got.joint_gradient.size() == 140 && got.min_direction.size() == 210);
    CHECK(got.pair_clearance.size() == 280 && got.fk_status.size() == 70 && got.min_pair.size() == 70);
    options.with_gradient = options.per_pair = false;
    const SelfCollisionChecks bare = CheckSelfCollision(model, tree, pairs, q, options);
    CHECK(bare.joint_gradient.empty() && bare.pair_clearance.empty() && bare.status == got.status);

    // the layer's calls that exist without this one: the poses, then the summed form on the call's own worst pair
    const LinkPoses poses = ComputeLinkPoses(tree, q, 70, nullptr, options.joint_limits);
    std::vector<double> weight(70 * 4, 0.0), gradient(70 * 4 * 3, 0.0);
    std::vector<restated::Configuration> want;
    for (size_t b = 0; b < 70; b++)
    {
      std::vector<double> centres;
      for (size_t s = 0; s < 4; s++)
      {
        const double* m = &poses.link_poses[(b * 3 + static_cast<size_t>(model.link[s])) * 16];
        for (size_t r = 0; r < 3; r++)
        {
          const volatile double x = m[r] * model.xyzr[s][0], y = m[4 + r] * model.xyzr[s][1], z = m[8 + r] * model.xyzr[s][2];
          const volatile double xy = x + y;
          const volatile double xyz = xy + z;
          centres.push_back(xyz + m[12 + r]);
        }
      }
      want.push_back(restated::Reduce(centres, radii, pairs, options.minimum_clearance, options.no_value_is_collision));
      if (got.min_pair[b] >= 0)
        for (int side = 0; side < 2; side++)
        {
          const size_t sphere = static_cast<size_t>(pairs[static_cast<size_t>(got.min_pair[b])][static_cast<size_t>(side)]);
          weight[b * 4 + sphere] = 1.0;
          for (size_t r = 0; r < 3; r++)
            gradient[(b * 4 + sphere) * 3 + r] = side == 0 ? got.min_direction[b * 3 + r] : -got.min_direction[b * 3 + r];
        }
    }
    const std::vector<double> summed = ClearanceJointGradient(tree, poses.link_poses, model, weight, gradient);
    int collisions = 0, clear = 0, no_value = 0, coincident = 0;
    for (size_t b = 0; b < 70; b++)
    {
      const restated::Configuration& w = want[b];
      bool same = got.status[b] == w.status && got.num_below[b] == w.num_below &&
                  got.num_without_value[b] == w.num_without_value && got.min_pair[b] == w.min_pair &&
                  SameDouble(got.min_clearance[b], w.min_clearance) && got.fk_status[b] == poses.status[b];
      for (size_t r = 0; r < 3; r++) same = same && SameDouble(got.min_direction[b * 3 + r], w.direction[r]);
      for (size_t p = 0; p < 4; p++) same = same && SameDouble(got.pair_clearance[b * 4 + p], w.clearance[p]);
      for (size_t j = 0; j < 2; j++)
        same = same && SameDouble(got.joint_gradient[b * 2 + j], w.min_pair < 0 ? restated::kNaN : summed[b * 2 + j]);
      // the formulas at the head of this file
      const double q0 = q[2 * b], q1 = q[2 * b + 1];
      if (std::isfinite(q0) && std::isfinite(q1))
      {
        const double sign = q0 > q1 ? 1.0 : -1.0;
        same = same && got.pair_clearance[b * 4] == 2.25 && got.pair_clearance[b * 4 + 1] == std::fabs(q0 - q1) - 0.75;
        if (q0 == q1)
          same = same && std::isnan(got.joint_gradient[b * 2]) && std::isnan(got.joint_gradient[b * 2 + 1]) &&
                 got.min_pair[b] == 1 && ++coincident > 0;
        else if (std::fabs(q0 - q1) < 3.0)
          same = same && got.min_pair[b] == 1 && got.min_direction[b * 3] == sign &&
                 got.joint_gradient[b * 2] == sign && got.joint_gradient[b * 2 + 1] == -sign;
      }
      if (!same)
      {
        std::printf("  configuration %zu (q %g %g) variant %d: status %d/%d below %d/%d without %d/%d pair %d/%d clearance "
                    "%g/%g gradient %g %g / %g %g\n",
                    b, q0, q1, variant, got.status[b], w.status, got.num_below[b], w.num_below, got.num_without_value[b],
                    w.num_without_value, got.min_pair[b], w.min_pair, got.min_clearance[b], w.min_clearance,
                    got.joint_gradient[b * 2], got.joint_gradient[b * 2 + 1], summed[b * 2], summed[b * 2 + 1]);
        CHECK(false);
      }
      collisions += got.status[b] == VGT_HIP_SELF_COLLISION;
      clear += got.status[b] == VGT_HIP_SELF_CLEAR;
      no_value += got.status[b] == VGT_HIP_SELF_NO_VALUE;
    }
    CHECK(collisions > 0 && clear > 0 && coincident > 0 && (no_value > 0) == (variant < 2));
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
