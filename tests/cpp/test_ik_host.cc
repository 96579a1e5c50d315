// KinematicChain and SolveInverseKinematics of the C++ host layer (include/vgt_hip/inverse_kinematics.hpp).  --no-device:
// the chain finder against chains written by hand, and the argument errors, none of which may ask for a device.  With a
// device: SolveInverseKinematics against answers derived by hand and against ComputeLinkPoses on the rows it returns.
//
// The hand-made tree.  Link 0 slides along x on the base (column 0); link 1 turns about z on link 0 (column 1); link 2,
// the tool, is fixed on link 1 at (1, 0, 0); link 3, a camera, is fixed on link 0.  The tool sits at
// (q0 + cos q1, sin q1, 0) and is turned by q1 about z.  At q = (0, 0) the columns are (0, 1, 0, 0, 0, 1) for link 1 and
// (1, 0, 0, 0, 0, 0) for link 0; with lambda = 1 and the target 0.5 further along x the system is A_00 = 2, b_0 = 0.5 with
// no coupling to the other rows, whose right-hand sides are zero: y = (0.25, 0, 0, 0, 0, 0) and dq = (0.25, 0), exactly.
#include <vgt_hip.h>
#include <vgt_hip/inverse_kinematics.hpp>

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

static KinematicTree HandTree()
{
  KinematicLink slide, turn, tool, camera;
  slide.joint_type = VGT_HIP_JOINT_PRISMATIC;
  slide.joint_index = 0;
  slide.axis = {{1.0, 0.0, 0.0}};
  turn.parent = 0;
  turn.joint_type = VGT_HIP_JOINT_REVOLUTE;
  turn.joint_index = 1;
  turn.axis = {{0.0, 0.0, 1.0}};
  tool.parent = 1;
  tool.origin = Isometry3::Translation(1.0, 0.0, 0.0);
  camera.parent = 0;
  camera.origin = Isometry3::Translation(0.0, 0.0, 0.5);
  return KinematicTree({slide, turn, tool, camera}, 2);
}

// n moving links in a row, one column each
static KinematicTree Serial(int n)
{
  std::vector<KinematicLink> links(static_cast<size_t>(n));
  for (int i = 0; i < n; i++)
  {
    links[static_cast<size_t>(i)].parent = i - 1;
    links[static_cast<size_t>(i)].joint_type = i % 2 ? VGT_HIP_JOINT_PRISMATIC : VGT_HIP_JOINT_REVOLUTE;
    links[static_cast<size_t>(i)].joint_index = i;
  }
  return KinematicTree(links, n);
}

static int RunNoDevice()
{
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const KinematicTree tree = HandTree();
  // the chain finder
  CHECK((KinematicChain(tree, 2) == std::vector<int32_t>{0, 1, 2}));
  CHECK((KinematicChain(tree, 3) == std::vector<int32_t>{0, 3}));
  CHECK((KinematicChain(tree, 0) == std::vector<int32_t>{0}));
  CHECK(ThrowsInvalidArgument([&] { KinematicChain(tree, 4); }, "tip link 4 is not in [0, 4)"));
  CHECK(ThrowsInvalidArgument([&] { KinematicChain(tree, -1); }, "tip link -1"));
  // argument errors of the layer, before a device is asked for
  const std::vector<Isometry3> targets(2);
  const std::vector<double> seeds(4, 0.0);
  const auto with = [&](const char* needle, const IkOptions& options, int32_t tip = 2) {
    return ThrowsInvalidArgument([&] { SolveInverseKinematics(tree, tip, targets, seeds, options); }, needle);
  };
  IkOptions options;
  CHECK(with("tip link 4", options, 4));
  CHECK(ThrowsInvalidArgument([&] { SolveInverseKinematics(tree, 2, targets, {0.0, 0.0, 0.0}); }, "one value per problem"));
  options.seeds_per_target = 2;
  CHECK(with("one value per problem", options));
  options.seeds_per_target = 0;
  CHECK(with("at least one target and one seed", options));
  options = IkOptions();
  options.max_iterations = -1;
  CHECK(with("max_iterations", options));
  options.max_iterations = 10001;
  CHECK(with("max_iterations", options));
  options = IkOptions();
  options.damping = -0.5;
  CHECK(with("damping", options));
  options.damping = nan;
  CHECK(with("damping", options));
  options = IkOptions();
  options.max_step = 0.0;
  CHECK(with("max_step", options));
  options.max_step = nan;
  CHECK(with("max_step", options));
  options = IkOptions();
  options.rotation_tolerance = -1.0;
  CHECK(with("tolerance", options));
  options = IkOptions();
  options.position_tolerance = nan;
  CHECK(with("tolerance", options));
  options = IkOptions();
  options.task_weights[4] = -1.0;
  CHECK(with("task weight", options));
  options.task_weights[4] = inf;
  CHECK(with("task weight", options));
  options = IkOptions();
  options.joint_limits = {0.0, 1.0};
  CHECK(with("joint_limits", options));
  // a mimic joint on the chain, and one off it
  {
    KinematicLink a, b, c;
    a.joint_type = VGT_HIP_JOINT_REVOLUTE;
    b.parent = 0;
    c.parent = 1;
    c.joint_type = VGT_HIP_JOINT_PRISMATIC;
    const KinematicTree mimic({a, b, c}, 1);
    CHECK(ThrowsInvalidArgument([&] { SolveInverseKinematics(mimic, 2, targets, {0.0, 0.0}); },
                                "links 0 and 2 on the chain to link 2 both read column 0"));
    // (tip 1: only link 0 moves; no targets: no device is needed)
    const IkSolutions none = SolveInverseKinematics(mimic, 1, {}, {});
    CHECK(none.joints.empty() && none.status.empty() && none.tip_pose.empty());
  }
  // the longest chain the kernel takes, and one link more
  {
    const int most = vgt_hip_ik_max_chain_joints();
    CHECK(most >= 16);
    const KinematicTree longest = Serial(most), longer = Serial(most + 1);
    CHECK(SolveInverseKinematics(longest, most - 1, {}, {}).status.empty());
    const std::string needle = std::to_string(most + 1) + " moving links";
    CHECK(ThrowsInvalidArgument(
        [&] { SolveInverseKinematics(longer, most, targets, std::vector<double>(2 * static_cast<size_t>(most + 1), 0.0)); },
        needle.c_str()));
    // (the link before the tip of the longer tree has a chain of `most` again)
    CHECK(SolveInverseKinematics(longer, most - 1, {}, {}).status.empty());
  }
  // the C ABI's own errors, before the context is looked at
  {
    double memory[64] = {};
    vgt_hip_ctx* stand_in = reinterpret_cast<vgt_hip_ctx*>(memory);
    uint8_t status[2] = {9, 9};
    CHECK(vgt_hip_solve_ik(stand_in, nullptr, 0, memory, 1, 1, memory, nullptr, nullptr, nullptr, 1, 0.0, 1.0, 0.0, 0.0,
                           nullptr, status, nullptr, nullptr, nullptr, nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "null argument") != nullptr);
    CHECK(vgt_hip_solve_ik_workspace_bytes(7, 100) == 5600 && vgt_hip_solve_ik_workspace_bytes(7, 0) == 0);
    CHECK(status[0] == 9 && status[1] == 9);
  }
  return g_failures;
}

static bool SameDouble(double a, double b)
{
  return (std::isnan(a) && std::isnan(b)) || std::memcmp(&a, &b, sizeof(double)) == 0;
}

static int RunDevice()
{
  const KinematicTree tree = HandTree();
  // by hand: the seed evaluated only, then one step with lambda = 1
  {
    IkOptions options;
    options.max_iterations = 0;
    const std::vector<Isometry3> target = {Isometry3::Translation(1.5, 0.0, 0.0)};
    IkSolutions got = SolveInverseKinematics(tree, 2, target, {0.0, 0.0}, options);
    CHECK(got.status.size() == 1 && got.status[0] == VGT_HIP_IK_ITERATION_LIMIT && got.iterations[0] == 0);
    CHECK(got.joints[0] == 0.0 && got.joints[1] == 0.0 && got.fk_status[0] == 0);
    CHECK(got.error[0] == 0.5 && got.error[1] == 0.0 && got.error[2] == 0.0 && got.error[5] == 0.0);
    CHECK(got.tip_pose[12] == 1.0 && got.tip_pose[0] == 1.0 && got.tip_pose[5] == 1.0 && got.tip_pose[15] == 1.0);
    options.max_iterations = 1;
    options.damping = 1.0;
    got = SolveInverseKinematics(tree, 2, target, {0.0, 0.0}, options);
    CHECK(got.status[0] == VGT_HIP_IK_ITERATION_LIMIT && got.iterations[0] == 1);
    CHECK(got.joints[0] == 0.25 && got.joints[1] == 0.0 && got.error[0] == 0.25 && got.tip_pose[12] == 1.25);
    options.max_step = 0.125;
    got = SolveInverseKinematics(tree, 2, target, {0.0, 0.0}, options);
    CHECK(got.joints[0] == 0.125 && got.tip_pose[12] == 1.125);
    options.joint_limits = {-1.0, 0.0625, -1.0, 1.0};
    got = SolveInverseKinematics(tree, 2, target, {0.0, 0.0}, options);
    CHECK(got.joints[0] == 0.0625 && got.fk_status[0] == 0);
    // the camera's chain has the slide alone: position-only along x it is there after one undamped step... which a
    // singular A refuses; with a little damping it converges
    options = IkOptions();
    options.task_weights = {{1.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
    options.damping = 0.0;
    got = SolveInverseKinematics(tree, 3, {Isometry3::Translation(2.0, 0.0, 0.5)}, {0.0, 0.0}, options);
    CHECK(got.status[0] == VGT_HIP_IK_DEGENERATE && got.iterations[0] == 0 && got.joints[0] == 0.0);
    options.damping = 1e-3;
    got = SolveInverseKinematics(tree, 3, {Isometry3::Translation(2.0, 0.0, 0.5)}, {0.0, 7.0}, options);
    CHECK(got.status[0] == VGT_HIP_IK_CONVERGED && std::fabs(got.joints[0] - 2.0) <= 1e-6 && got.joints[1] == 7.0);
  }
  // 70 reachable targets, three seeds each: the rows, put through ComputeLinkPoses, give the tip poses bit for bit
  {
    std::vector<double> truth;
    for (int t = 0; t < 70; t++)
    {
      truth.push_back(0.125 * ((t * 7) % 23) - 1.0);
      truth.push_back(0.05 * ((t * 5) % 41) - 1.0);
    }
    const LinkPoses at_truth = ComputeLinkPoses(tree, truth, 70);
    std::vector<Isometry3> targets(70);
    std::vector<double> seeds;
    for (size_t t = 0; t < 70; t++)
    {
      for (size_t e = 0; e < 16; e++) targets[t].m[e] = at_truth.link_poses[(t * 4 + 2) * 16 + e];
      for (int r = 0; r < 3; r++)
      {
        seeds.push_back(truth[2 * t] + 0.1 * (r - 1));
        seeds.push_back(truth[2 * t + 1] - 0.2 * (r - 1));
      }
    }
    seeds[2 * 5] = std::numeric_limits<double>::quiet_NaN();
    IkOptions options;
    options.seeds_per_target = 3;
    const IkSolutions got = SolveInverseKinematics(tree, 2, targets, seeds, options);
    CHECK(got.status.size() == 210 && got.joints.size() == 420 && got.tip_pose.size() == 210 * 16);
    const LinkPoses back = ComputeLinkPoses(tree, got.joints, 210);
    int converged = 0, at_seed = 0;
    for (size_t b = 0; b < 210; b++)
    {
      bool same = true;
      for (size_t e = 0; e < 16; e++) same = same && SameDouble(got.tip_pose[b * 16 + e], back.link_poses[(b * 4 + 2) * 16 + e]);
      same = same && got.fk_status[b] == back.status[b];
      if (b == 5)
        same = same && got.status[b] == VGT_HIP_IK_NOT_COMPUTABLE && std::isnan(got.joints[10]) && got.iterations[b] == 0;
      else if (got.status[b] == VGT_HIP_IK_CONVERGED)
      {
        converged++;
        at_seed += got.iterations[b] == 0;
        for (size_t k = 0; k < 6; k++) same = same && std::fabs(got.error[b * 6 + k]) <= 1e-6;
        same = same && std::fabs(got.joints[2 * b] - truth[2 * (b / 3)]) <= 1e-5 &&
               std::fabs(got.joints[2 * b + 1] - truth[2 * (b / 3) + 1]) <= 1e-5;
      }
      if (!same)
      {
        std::printf("  problem %zu: status %d after %d steps, joints %g %g, truth %g %g\n", b, got.status[b],
                    got.iterations[b], got.joints[2 * b], got.joints[2 * b + 1], truth[2 * (b / 3)], truth[2 * (b / 3) + 1]);
        CHECK(false);
      }
    }
    std::printf("converged %d of 210, %d of them at the seed\n", converged, at_seed);
    CHECK(converged >= 200 && at_seed >= 69);
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
