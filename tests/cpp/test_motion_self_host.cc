// CheckMotionsWithSelf of the C++ host layer (include/vgt_hip/motion_self_queries.hpp).  --no-device: the argument errors
// of the layer and of the C ABI that need no device.  With a device and a file name: the motions, the thresholds and the
// answers in that file -- tests/test_cpp_motion_self.py computes them with tests/motion_self_ref.py on the same scene and
// writes them as hexadecimal doubles -- against what the layer returns, bit for bit, with and without the stop flag, and
// the form without a field and the form without pairs against the same file's answers for them.
//
// The scene (tests/test_cpp_motion_self.py builds the same).  Field: 8 x 4 x 4 cells of resolution 1, sdf[x, y, z] =
// x + 1.5.  Tree: the links 0 and 1 slide along x from (0, 1.5, 1.5), each with a joint of its own (q0, q1); link 2 is
// fixed on link 1 at (0, 0.5, 0).  Sphere 0 on link 0, radius 0.25; sphere 1 on link 1, radius 0.25; sphere 2 on link 2,
// radius 0.125.  Pairs: (0, 1) and (0, 2).
#include <vgt_hip.h>
#include <vgt_hip/motion_self_queries.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
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
  first.origin = Isometry3::Translation(0.0, 1.5, 1.5);
  second = first;
  second.joint_index = 1;
  bar.parent = 1;
  bar.joint_type = VGT_HIP_JOINT_FIXED;
  bar.origin = Isometry3::Translation(0.0, 0.5, 0.0);
  return KinematicTree({first, second, bar}, 2);
}

static SphereModel ThreeSpheres()
{
  SphereModel model;
  model.link = {0, 1, 2};
  model.xyzr = {{{0.0, 0.0, 0.0, 0.25}}, {{0.0, 0.0, 0.0, 0.25}}, {{0.0, 0.0, 0.0, 0.125}}};
  return model;
}

static SignedDistanceField Ramp()
{
  SignedDistanceField sdf;
  sdf.grid = DenseGrid(Isometry3::Identity(), "f", 1.0, 8, 4, 4, 0.0f);
  for (int64_t x = 0; x < 8; x++)
    for (int64_t y = 0; y < 4; y++)
      for (int64_t z = 0; z < 4; z++) sdf.grid.SetIndex(x, y, z, static_cast<float>(x) + 1.5f);
  return sdf;
}

static const std::vector<SpherePair> kPairs = {{{0, 1}}, {{0, 2}}};

static int RunNoDevice()
{
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const KinematicTree tree = ThreeLinks();
  const SphereModel model = ThreeSpheres();
  const SignedDistanceField sdf = Ramp();
  const std::vector<double> a = {1.0, 2.0}, b = {3.0, 4.0};
  CHECK(ThrowsInvalidArgument([&] { CheckMotionsWithSelf(nullptr, model, tree, {}, a, b, {2}); },
                              "neither a field nor a pair"));
  const SignedDistanceField empty;
  CHECK(ThrowsInvalidArgument([&] { CheckMotionsWithSelf(&empty, model, tree, kPairs, a, b, {2}); }, "initialized"));
  MotionSelfOptions options;
  options.minimum_clearance = nan;
  CHECK(ThrowsInvalidArgument([&] { CheckMotionsWithSelf(&sdf, model, tree, kPairs, a, b, {2}, options); },
                              "minimum_clearance must not be NaN"));
  options = MotionSelfOptions();
  options.self_minimum_clearance = nan;
  CHECK(ThrowsInvalidArgument([&] { CheckMotionsWithSelf(&sdf, model, tree, kPairs, a, b, {2}, options); },
                              "self_minimum_clearance must not be NaN"));
  options = MotionSelfOptions();
  options.joint_limits = {0.0};
  CHECK(ThrowsInvalidArgument([&] { CheckMotionsWithSelf(&sdf, model, tree, kPairs, a, b, {2}, options); },
                              "joint_limits"));
  CHECK(ThrowsInvalidArgument([&] { CheckMotionsWithSelf(&sdf, model, tree, kPairs, a, {3.0}, {2}); },
                              "one value per motion and joint"));
  CHECK(ThrowsInvalidArgument([&] { CheckMotionsWithSelf(&sdf, model, tree, kPairs, a, b, {2, 3}); },
                              "one count per motion"));
  CHECK(ThrowsInvalidArgument([&] { CheckMotionsWithSelf(&sdf, model, tree, kPairs, a, b, {-3}); },
                              "motion 0: num_steps -3"));
  SphereModel bad = model;
  bad.link.pop_back();
  CHECK(ThrowsInvalidArgument([&] { CheckMotionsWithSelf(&sdf, bad, tree, kPairs, a, b, {2}); }, "one link and one"));
  // no motions: no device is needed
  CHECK(CheckMotionsWithSelf(&sdf, model, tree, kPairs, {}, {}, {2}).empty());
  CHECK(vgt_hip_motion_self_tile_samples(1, 0) == 64 && vgt_hip_motion_self_tile_samples(664, 0) == 1 &&
        vgt_hip_motion_self_tile_samples(665, 0) == 0 && vgt_hip_motion_self_tile_samples(1, 1990) == 0);
  // the C ABI's own errors, before the context is looked at
  {
    double memory[64] = {};
    vgt_hip_ctx* stand_in = reinterpret_cast<vgt_hip_ctx*>(memory);
    const vgt_hip_kinematics* handle = reinterpret_cast<const vgt_hip_kinematics*>(memory);
    uint8_t status[2] = {9, 9};
    const auto call = [&](const float* field, int64_t num_pairs, uint32_t flags, int64_t motions) {
      return vgt_hip_check_motions_with_self(stand_in, field, 4, 4, 4, 1.0, nullptr, nullptr, nullptr, nullptr, 0,
                                             reinterpret_cast<const int32_t*>(memory), num_pairs, handle, memory, memory,
                                             nullptr, 2, motions, nullptr, nullptr, 0.0, 0.0, flags, status, nullptr,
                                             nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                             nullptr);
    };
    const float* field = reinterpret_cast<const float*>(memory);
    CHECK(call(nullptr, 0, 0, 2) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "neither a field nor a pair") != nullptr);
    CHECK(call(field, 1, 8, 2) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "unknown motion check flag") != nullptr);
    CHECK(call(field, -1, 0, 2) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(call(field, 1, 7, 0) == VGT_HIP_OK);
    CHECK(status[0] == 9 && status[1] == 9);
  }
  return g_failures;
}

static bool ReadDouble(std::FILE* file, double* value)
{
  char word[64];
  if (std::fscanf(file, "%63s", word) != 1) return false;
  *value = std::strtod(word, nullptr);
  return true;
}

static bool ReadChecks(std::FILE* file, size_t motions, std::vector<MotionSelfCheck>* out)
{
  out->resize(motions);
  for (MotionSelfCheck& c : *out)
  {
    int status, cause, fk;
    if (std::fscanf(file, "%d %d %d", &status, &c.first_collision, &cause) != 3) return false;
    if (!ReadDouble(file, &c.min_clearance)) return false;
    if (std::fscanf(file, "%d %d", &c.min_sample, &c.min_sphere) != 2) return false;
    for (double& g : c.min_gradient)
      if (!ReadDouble(file, &g)) return false;
    if (!ReadDouble(file, &c.self_min_clearance)) return false;
    if (std::fscanf(file, "%d %d %d", &c.self_min_sample, &c.self_min_pair, &fk) != 3) return false;
    c.status = static_cast<uint8_t>(status);
    c.collision_cause = static_cast<uint8_t>(cause);
    c.fk_status = static_cast<uint8_t>(fk);
  }
  return true;
}

static void Compare(const std::vector<MotionSelfCheck>& got, const std::vector<MotionSelfCheck>& want, const char* what)
{
  CHECK(got.size() == want.size());
  for (size_t e = 0; e < got.size() && e < want.size(); e++)
  {
    const MotionSelfCheck &g = got[e], &w = want[e];
    bool same = g.status == w.status && g.first_collision == w.first_collision &&
                g.collision_cause == w.collision_cause && SameDouble(g.min_clearance, w.min_clearance) &&
                g.min_sample == w.min_sample && g.min_sphere == w.min_sphere &&
                SameDouble(g.self_min_clearance, w.self_min_clearance) && g.self_min_sample == w.self_min_sample &&
                g.self_min_pair == w.self_min_pair && g.fk_status == w.fk_status;
    for (size_t r = 0; r < 3; r++) same = same && SameDouble(g.min_gradient[r], w.min_gradient[r]);
    if (!same)
    {
      std::printf("  %s, motion %zu: status %d/%d first %d/%d cause %d/%d clearance %g/%g sample %d/%d sphere %d/%d self "
                  "%g/%g sample %d/%d pair %d/%d fk %d/%d\n",
                  what, e, g.status, w.status, g.first_collision, w.first_collision, g.collision_cause, w.collision_cause,
                  g.min_clearance, w.min_clearance, g.min_sample, w.min_sample, g.min_sphere, w.min_sphere,
                  g.self_min_clearance, w.self_min_clearance, g.self_min_sample, w.self_min_sample, g.self_min_pair,
                  w.self_min_pair, g.fk_status, w.fk_status);
      CHECK(false);
    }
  }
}

// The file: "E minimum_clearance self_minimum_clearance lower0 upper0 lower1 upper1", then per motion "a0 a1 b0 b1 n",
// then six blocks of E answers: (both parts, field only, pairs only) x (all samples, stop at collision).
static int RunDevice(const char* path)
{
  std::FILE* file = std::fopen(path, "r");
  if (!file)
  {
    std::printf("cannot open %s\n", path);
    return 1;
  }
  int motions = 0;
  MotionSelfOptions options;
  options.joint_limits.resize(4);
  bool ok = std::fscanf(file, "%d", &motions) == 1 && motions > 0 && ReadDouble(file, &options.minimum_clearance) &&
            ReadDouble(file, &options.self_minimum_clearance);
  for (double& limit : options.joint_limits) ok = ok && ReadDouble(file, &limit);
  std::vector<double> from, to;
  std::vector<int32_t> steps;
  for (int e = 0; ok && e < motions; e++)
  {
    double a0, a1, b0, b1;
    int n;
    ok = ReadDouble(file, &a0) && ReadDouble(file, &a1) && ReadDouble(file, &b0) && ReadDouble(file, &b1) &&
         std::fscanf(file, "%d", &n) == 1;
    from.insert(from.end(), {a0, a1});
    to.insert(to.end(), {b0, b1});
    steps.push_back(n);
  }
  std::vector<MotionSelfCheck> want[3][2];
  for (int form = 0; form < 3; form++)
    for (int stop = 0; stop < 2; stop++) ok = ok && ReadChecks(file, static_cast<size_t>(motions), &want[form][stop]);
  std::fclose(file);
  CHECK(ok);
  if (!ok) return g_failures;

  const KinematicTree tree = ThreeLinks();
  const SphereModel model = ThreeSpheres();
  const SignedDistanceField sdf = Ramp();
  int collisions = 0, causes = 0;
  for (int stop = 0; stop < 2; stop++)
  {
    options.stop_at_collision = stop != 0;
    const std::vector<MotionSelfCheck> both = CheckMotionsWithSelf(&sdf, model, tree, kPairs, from, to, steps, options);
    Compare(both, want[0][stop], stop ? "both parts, stop" : "both parts");
    Compare(CheckMotionsWithSelf(&sdf, model, tree, {}, from, to, steps, options), want[1][stop], "the field alone");
    Compare(CheckMotionsWithSelf(nullptr, model, tree, kPairs, from, to, steps, options), want[2][stop],
            "the pairs alone");
    for (const MotionSelfCheck& c : both)
    {
      collisions += c.status == VGT_HIP_MOTION_COLLISION;
      causes |= c.collision_cause;
    }
  }
  CHECK(collisions > 0 && causes == 3);
  return g_failures;
}

int main(int argc, char** argv)
{
  const bool no_device = argc > 1 && std::strcmp(argv[1], "--no-device") == 0;
  int failures = RunNoDevice();
  if (!no_device)
  {
    if (argc < 2)
    {
      std::printf("usage: test_motion_self_host --no-device | <file of motions and answers>\n");
      return 2;
    }
    failures = RunDevice(argv[1]);
  }
  if (failures == 0) std::printf("PASSED\n");
  return failures == 0 ? 0 : 1;
}
