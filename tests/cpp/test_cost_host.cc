// ClearanceCost of the C++ host layer (include/vgt_hip/clearance_cost.hpp).  --no-device: the restatement in this file
// (the hinge and the ordered sums, over per-sphere values) against answers derived by hand on a two-link tree, and the
// argument errors.  With a device: ClearanceCost against the hand-made answers and against that restatement over the
// per-sphere values of CheckSphereModel from joint values, with ClearanceJointGradient's summed form on the poses of
// ComputeLinkPoses for the gradient, bit for bit; then all of it once more with the grid on a turned and shifted origin
// and the tree's base on that origin, against the identity grid's run.
//
// The hand-made scene (that of test_motion_host.cc).  Field: 8 x 4 x 4 cells of resolution 1, sdf[x][y][z] = x + 1.5: the
// estimate at a point p with 0.5 <= p_x <= 7.5 is p_x + 0.5 and its gradient (1, 0, 0).  Tree: link 0 prismatic along x at
// (0, 1.5, 1.5), link 1 fixed on it at (1, 0, 0).  Sphere 0 on link 1, radius 0.25: clearance q + 1.25; sphere 1 on link
// 0, radius 0: clearance q + 0.5.  Both move with the one joint: the term of either sphere is 1, the gradient w_0 + w_1.
#include <vgt_hip.h>
#include <vgt_hip/clearance_cost.hpp>

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

// the header's hinge; false: d is NaN, no contribution
static bool Hinge(double d, double eps, double* c, double* w)
{
  *c = kNaN;
  *w = 0.0;
  if (std::isnan(d)) return false;
  if (d < 0.0)
  {
    const volatile double half = eps * 0.5;
    *c = half - d;
    *w = -1.0;
  }
  else if (d <= eps)
  {
    const volatile double t = d - eps;
    const volatile double square = t * t;
    const volatile double halved = square * 0.5;
    *c = halved / eps;
    *w = t / eps;
  }
  else
    *c = 0.0;
  return true;
}

// one configuration's outputs but the gradient, from its spheres' clearances and gradients; weight: what the summed
// form takes
struct Configuration
{
  double cost = 0.0;
  int32_t num_active = 0, num_outside = 0, num_without_gradient = 0;
  std::vector<double> weight;
};

static Configuration Reduce(const double* clearance, const double* gradient, size_t spheres, double eps)
{
  Configuration out;
  for (size_t s = 0; s < spheres; s++)
  {
    double c, w;
    if (!Hinge(clearance[s], eps, &c, &w))
    {
      out.num_outside++;
      out.weight.push_back(0.0);
      continue;
    }
    const volatile double sum = out.cost + c;
    out.cost = sum;
    if (w != 0.0)
    {
      out.num_active++;
      if (std::isnan(gradient[3 * s]) || std::isnan(gradient[3 * s + 1]) || std::isnan(gradient[3 * s + 2]))
      {
        out.num_without_gradient++;
        w = 0.0;
      }
    }
    out.weight.push_back(w);
  }
  return out;
}

// The hand-made scene at joint value q (a multiple of 0.5), by the formulas at the head of this file.
struct Hand
{
  Configuration reduced;
  double joint_gradient;
  uint8_t fk_status;
};

static Hand HandConfiguration(double q, double eps, const double* limits)
{
  const bool usable = std::isfinite(q);
  const double x[2] = {q + 1.0, q};  // the spheres' centres
  const double radius[2] = {0.25, 0.0};
  double clearance[2], gradient[6];
  for (int s = 0; s < 2; s++)
  {
    const bool value = usable && x[s] >= 0.5 && x[s] <= 7.5;
    clearance[s] = value ? (x[s] + 0.5) - radius[s] : kNaN;
    gradient[3 * s] = value ? 1.0 : kNaN;
    gradient[3 * s + 1] = gradient[3 * s + 2] = value ? 0.0 : kNaN;
  }
  Hand out;
  out.reduced = Reduce(clearance, gradient, 2, eps);
  const volatile double first = 0.0 + out.reduced.weight[0] * 1.0;
  out.joint_gradient = first + out.reduced.weight[1] * 1.0;
  out.fk_status = static_cast<uint8_t>((usable ? 0 : 1) | (limits && (q < limits[0] || q > limits[1]) ? 2 : 0));
  return out;
}
}  // namespace restated

static bool SameDouble(double a, double b)
{
  return (std::isnan(a) && std::isnan(b)) || std::memcmp(&a, &b, sizeof(double)) == 0;
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
  using restated::HandConfiguration;
  using restated::Hinge;
  const double nan = restated::kNaN, inf = std::numeric_limits<double>::infinity();
  // the hinge at its edges, eps = 0.25
  {
    double c, w;
    CHECK(Hinge(-1.0, 0.25, &c, &w) && c == 1.125 && w == -1.0);
    CHECK(Hinge(-0.0, 0.25, &c, &w) && c == 0.125 && w == -1.0);  // (-0.0 < 0 is false: the second branch)
    CHECK(Hinge(0.0, 0.25, &c, &w) && c == 0.125 && w == -1.0);
    CHECK(Hinge(0.125, 0.25, &c, &w) && c == 0.03125 && w == -0.5);
    CHECK(Hinge(0.25, 0.25, &c, &w) && c == 0.0 && w == 0.0 && !std::signbit(c) && !std::signbit(w));
    CHECK(Hinge(std::nextafter(0.25, 1.0), 0.25, &c, &w) && c == 0.0 && w == 0.0);
    CHECK(Hinge(inf, 0.25, &c, &w) && c == 0.0 && w == 0.0);
    CHECK(Hinge(-inf, 0.25, &c, &w) && c == inf && w == -1.0);
    CHECK(!Hinge(nan, 0.25, &c, &w) && w == 0.0);
  }
  // q = 0.5: clearances 1.75 and 1.0; with eps = 2: t = -0.25 and -1, c = 0.015625 and 0.25, w = -0.125 and -0.5
  {
    const restated::Hand hand = HandConfiguration(0.5, 2.0, nullptr);
    CHECK(hand.reduced.cost == 0.265625 && hand.joint_gradient == -0.625 && hand.reduced.num_active == 2);
    CHECK(hand.reduced.num_outside == 0 && hand.reduced.num_without_gradient == 0 && hand.fk_status == 0);
  }
  // q = 7: sphere 0 at x = 8 has no value; sphere 1: clearance 7.5, beyond the margin
  {
    const restated::Hand hand = HandConfiguration(7.0, 2.0, nullptr);
    CHECK(hand.reduced.cost == 0.0 && hand.joint_gradient == 0.0 && hand.reduced.num_active == 0);
    CHECK(hand.reduced.num_outside == 1);
    const double limits[2] = {0.0, 6.0};
    CHECK(HandConfiguration(7.0, 2.0, limits).fk_status == 2 && HandConfiguration(inf, 2.0, limits).fk_status == 3);
    CHECK(HandConfiguration(nan, 2.0, nullptr).reduced.num_outside == 2 && HandConfiguration(nan, 2.0, limits).fk_status == 1);
  }
  // the NaN-gradient rule: an active sphere with a NaN gradient counts in the cost, not in the gradient
  {
    const double clearance[3] = {0.125, 0.125, 0.5}, gradient[9] = {1.0, 0.0, 0.0, 0.0, nan, 0.0, nan, nan, nan};
    const restated::Configuration got = restated::Reduce(clearance, gradient, 3, 0.25);
    CHECK(got.cost == 0.0625 && got.num_active == 2 && got.num_without_gradient == 1 && got.num_outside == 0);
    CHECK(got.weight[0] == -0.5 && got.weight[1] == 0.0 && got.weight[2] == 0.0);
  }

  // argument errors of the layer, before a device is asked for
  {
    const KinematicTree tree = TwoLinks();
    const SphereModel model = TwoSpheres();
    const SignedDistanceField sdf = Ramp();
    CHECK(ThrowsInvalidArgument([&] { ClearanceCost(SignedDistanceField(), model, tree, {0.0}, 0.25); }, "initialized"));
    for (const double margin : {0.0, -0.25, inf, nan})
      CHECK(ThrowsInvalidArgument([&] { ClearanceCost(sdf, model, tree, {0.0}, margin); },
                                  "margin must be positive and finite"));
    CHECK(ThrowsInvalidArgument([&] { ClearanceCost(sdf, model, tree, {0.0, 1.0}, 0.25, {}, 3); },
                                "one value per configuration and joint"));
    ClearanceCostOptions options;
    options.joint_limits = {0.0};
    CHECK(ThrowsInvalidArgument([&] { ClearanceCost(sdf, model, tree, {0.0}, 0.25, options); }, "joint_limits"));
    SphereModel bad = model;
    bad.link[1] = 2;
    CHECK(ThrowsInvalidArgument([&] { ClearanceCost(sdf, bad, tree, {0.0}, 0.25); }, "sphere 1: link 2 is not in"));
    bad = model;
    bad.xyzr[0][3] = -1.0;
    CHECK(ThrowsInvalidArgument([&] { ClearanceCost(sdf, bad, tree, {0.0}, 0.25); }, "sphere 0: the radius"));
    bad = model;
    bad.link.pop_back();
    CHECK(ThrowsInvalidArgument([&] { ClearanceCost(sdf, bad, tree, {0.0}, 0.25); }, "one link and one"));
    // no configurations: no device is needed
    const ClearanceCosts none = ClearanceCost(sdf, model, tree, {}, 0.25);
    CHECK(none.cost.empty() && none.joint_gradient.empty() && none.fk_status.empty());
    CHECK(vgt_hip_cost_tile_samples(1) == 64 && vgt_hip_cost_tile_samples(512) == 1 && vgt_hip_cost_tile_samples(513) == 0);
  }

  // the C ABI's own errors, before the context is looked at
  {
    double memory[64] = {};
    vgt_hip_ctx* stand_in = reinterpret_cast<vgt_hip_ctx*>(memory);
    const vgt_hip_kinematics* handle = reinterpret_cast<const vgt_hip_kinematics*>(memory);
    const float field[8] = {};
    double cost[2] = {9.0, 9.0};
    CHECK(vgt_hip_clearance_cost(stand_in, field, 2, 2, 2, 1.0, nullptr, nullptr, nullptr, nullptr, 0, handle, memory, 2,
                                 nullptr, nullptr, 0.0, 0, cost, nullptr, nullptr, nullptr, nullptr,
                                 nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "margin must be positive and finite") != nullptr);
    CHECK(vgt_hip_clearance_cost(stand_in, field, 2, 2, 2, 1.0, nullptr, nullptr, nullptr, nullptr, 0, handle, memory, 2,
                                 nullptr, nullptr, 0.25, 1, cost, nullptr, nullptr, nullptr, nullptr,
                                 nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "unknown clearance cost flag") != nullptr);
    CHECK(vgt_hip_clearance_cost(stand_in, field, 2, 2, 2, 1.0, nullptr, nullptr, nullptr, nullptr, 0, handle, nullptr, 0,
                                 nullptr, nullptr, 0.25, 0, cost, nullptr, nullptr, nullptr, nullptr, nullptr) == VGT_HIP_OK);
    CHECK(cost[0] == 9.0 && cost[1] == 9.0);
  }
  return g_failures;
}

static int RunDevice()
{
  const KinematicTree tree = TwoLinks();
  const SphereModel model = TwoSpheres();
  const SignedDistanceField identity_sdf = Ramp();
  const Isometry3 origin = TurnedOrigin();
  // 70 configurations of the hand-made scene at multiples of 0.5, on both sides of the grid's ends and of the margin
  std::vector<double> q;
  for (int b = 0; b < 70; b++) q.push_back(0.5 * ((b * 7) % 23) - 2.0);
  q[11] = std::numeric_limits<double>::quiet_NaN();
  q[12] = std::numeric_limits<double>::infinity();
  // The second pass: the ramp on the turned and shifted origin and the tree's base on that origin, so that the tree is
  // where it was in the grid.  The comparisons with the layer's other calls stay bit for bit; the answers by hand give
  // way to the identity grid's run of the same call, which they hold.  There the margins are off the lattice of the
  // clearances (multiples of 0.25): a clearance equal to the margin has w == +0.0 and is not active, and the rounding of
  // the two more transforms would decide on which side of it the turned run lands.
  for (int turned = 0; turned < 2; turned++)
  {
    const SignedDistanceField sdf = turned ? Ramp(origin) : identity_sdf;
    int compared = 0, on_an_end_face = 0;
    for (int variant = 0; variant < 4; variant++)
    {
      // (clearances start at 1: a smaller margin has no active sphere)
      const double margin = ((variant & 1) ? 2.0 : 4.0) + (turned ? 0.125 : 0.0);
      ClearanceCostOptions options;
      if (variant >= 2) options.joint_limits = {0.0, 6.0};
      const ClearanceCostOptions plain_options = options;
      if (turned)
      {
        options.has_world_from_base = true;
        options.world_from_base = origin;
      }
      const ClearanceCosts got = ClearanceCost(sdf, model, tree, q, margin, options);
      CHECK(got.cost.size() == 70 && got.joint_gradient.size() == 70 && got.num_active.size() == 70);
      CHECK(got.num_outside.size() == 70 && got.num_without_gradient.size() == 70 && got.fk_status.size() == 70);
      options.with_gradient = false;
      const ClearanceCosts scored = ClearanceCost(sdf, model, tree, q, margin, options);
      CHECK(scored.joint_gradient.empty() && scored.num_without_gradient.empty() && scored.cost.size() == 70);

      // the layer's calls that exist without this one
      JointSphereModelOptions flat_options;
      flat_options.per_sphere = true;
      flat_options.joint_limits = options.joint_limits;
      flat_options.has_world_from_base = options.has_world_from_base;
      flat_options.world_from_base = options.world_from_base;
      const JointSphereModelChecks flat = CheckSphereModel(sdf, model, tree, q, flat_options);
      const LinkPoses poses = ComputeLinkPoses(tree, q, 70, turned ? &origin : nullptr, options.joint_limits);
      std::vector<double> weights;
      std::vector<restated::Configuration> reduced;
      for (size_t b = 0; b < 70; b++)
      {
        reduced.push_back(restated::Reduce(&flat.checks.sphere_clearance[2 * b], &flat.checks.sphere_gradient[6 * b], 2, margin));
        weights.insert(weights.end(), reduced.back().weight.begin(), reduced.back().weight.end());
      }
      const std::vector<double> summed = ClearanceJointGradient(tree, poses.link_poses, model, weights, flat.checks.sphere_gradient);
      // the same call on the identity grid
      const ClearanceCosts plain = turned ? ClearanceCost(identity_sdf, model, tree, q, margin, plain_options) : got;
      int active = 0, outside = 0;
      for (size_t b = 0; b < 70; b++)
      {
        const bool in_hand_range = std::isnan(q[b]) || std::isinf(q[b]) || (q[b] >= 0.5 && q[b] <= 6.5) || q[b] > 7.5 || q[b] < -1.5;
        const restated::Hand hand = restated::HandConfiguration(q[b], margin, options.joint_limits.empty() ? nullptr : options.joint_limits.data());
        const restated::Configuration& want = reduced[b];
        const bool same = SameDouble(got.cost[b], want.cost) && SameDouble(got.joint_gradient[b], summed[b]) &&
                          got.num_active[b] == want.num_active && got.num_outside[b] == want.num_outside &&
                          got.num_without_gradient[b] == want.num_without_gradient && got.fk_status[b] == flat.fk_status[b];
        // (the formulas at the head of this file hold where both spheres are well inside the grid, or both outside)
        const bool same_as_hand = turned || !in_hand_range ||
                                  (SameDouble(got.cost[b], hand.reduced.cost) && SameDouble(got.joint_gradient[b], hand.joint_gradient) &&
                                   got.num_active[b] == hand.reduced.num_active && got.num_outside[b] == hand.reduced.num_outside &&
                                   got.fk_status[b] == hand.fk_status);
        if (!same || !same_as_hand)
        {
          std::printf("  configuration %zu (q %g) variant %d turned %d: cost %g/%g/%g gradient %g/%g/%g active %d/%d outside %d/%d fk %d/%d\n",
                      b, q[b], variant, turned, got.cost[b], want.cost, hand.reduced.cost, got.joint_gradient[b], summed[b],
                      hand.joint_gradient, got.num_active[b], want.num_active, got.num_outside[b], want.num_outside,
                      got.fk_status[b], flat.fk_status[b]);
          CHECK(false);
        }
        CHECK(SameDouble(scored.cost[b], got.cost[b]) && scored.num_active[b] == got.num_active[b] &&
              scored.num_outside[b] == got.num_outside[b] && scored.fk_status[b] == got.fk_status[b]);
        active += got.num_active[b];
        outside += got.num_outside[b];
        if (!turned) continue;
        // A sphere centre on an end face of the grid in x (the spheres are at q + 1 and q) is inside or outside by the
        // rounding of the transforms; every other configuration is the identity grid's, up to that rounding.
        if (q[b] == -1.0 || q[b] == 0.0 || q[b] == 7.0 || q[b] == 8.0)
        {
          on_an_end_face++;
          continue;
        }
        compared++;
        const auto close = [](double a, double b) {
          return (std::isnan(a) && std::isnan(b)) || a == b || std::fabs(a - b) <= 1e-12;
        };
        const bool as_plain = close(got.cost[b], plain.cost[b]) && close(got.joint_gradient[b], plain.joint_gradient[b]) &&
                              got.num_active[b] == plain.num_active[b] && got.num_outside[b] == plain.num_outside[b] &&
                              got.num_without_gradient[b] == plain.num_without_gradient[b] &&
                              got.fk_status[b] == plain.fk_status[b];
        if (!as_plain)
        {
          std::printf("  configuration %zu (q %g) variant %d, turned/identity: cost %.17g/%.17g gradient %.17g/%.17g active %d/%d outside %d/%d fk %d/%d\n",
                      b, q[b], variant, got.cost[b], plain.cost[b], got.joint_gradient[b], plain.joint_gradient[b],
                      got.num_active[b], plain.num_active[b], got.num_outside[b], plain.num_outside[b], got.fk_status[b],
                      plain.fk_status[b]);
          CHECK(false);
        }
      }
      CHECK(active > 0 && outside > 0);
    }
    // per variant the 12 configurations with q in {-1, 0, 7, 8}
    if (turned) CHECK(on_an_end_face == 4 * 12 && compared == 4 * (70 - 12));
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
