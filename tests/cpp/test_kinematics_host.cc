// KinematicTree, ComputeLinkPoses, ClearanceJointGradient and CheckSphereModel from joint values of the C++ host layer
// (include/vgt_hip/kinematics.hpp) against an in-file restatement of vgt_hip_forward_kinematics and
// vgt_hip_clearance_joint_gradient (include/vgt_hip.h), bit for bit.
//   test_kinematics_host              the restatement against hand-derived answers, the argument errors, and the layer
//                                     on device 0 against the restatement
//   test_kinematics_host --no-device  the first two only: nothing here touches a device
#include <vgt_hip.h>
#include <vgt_hip/kinematics.hpp>

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

// ---- the restatement: every step in the order include/vgt_hip.h gives, one configuration at a time ----
namespace restated
{
const double kNaN = std::numeric_limits<double>::quiet_NaN();

static void SinCos(double q, double& s, double& c)
{
  const double k = std::nearbyint(q * 0x1.45f306dc9c883p-1);
  const double r = ((q - k * 0x1.921fb54400000p+0) - k * 0x1.0b4611a600000p-34) - k * 0x1.3198a2e037073p-69;
  const double z = r * r;
  const double S[8] = {0x1.952c77030ad4ap-49,  -0x1.ae7f3e733b81fp-41, 0x1.6124613a86d09p-33, -0x1.ae64567f544e4p-26,
                       0x1.71de3a556c734p-19,  -0x1.a01a01a01a01ap-13, 0x1.1111111111111p-7,  -0x1.5555555555555p-3};
  const double C[8] = {0x1.ae7f3e733b81fp-45,  -0x1.93974a8c07c9dp-37, 0x1.1eed8eff8d898p-29, -0x1.27e4fb7789f5cp-22,
                       0x1.a01a01a01a01ap-16,  -0x1.6c16c16c16c17p-10, 0x1.5555555555555p-5,  -0x1.0000000000000p-1};
  double ps = S[0], pc = C[0];
  for (int n = 1; n < 8; n++)
  {
    const double scaled = ps * z;
    ps = scaled + S[n];
  }
  for (int n = 1; n < 8; n++)
  {
    const double scaled = pc * z;
    pc = scaled + C[n];
  }
  const double cubed = r * z, tail = cubed * ps, even = z * pc;
  const double sin_r = r + tail, cos_r = 1.0 + even;
  switch (static_cast<long long>(k) & 3)
  {
    case 0: s = sin_r, c = cos_r; break;
    case 1: s = cos_r, c = -sin_r; break;
    case 2: s = -sin_r, c = -cos_r; break;
    default: s = -cos_r, c = sin_r; break;
  }
}

// 16 doubles column-major; only the twelve used elements are formed
static void Product(const double* a, const double* b, double* out)
{
  for (int r = 0; r < 3; r++)
  {
    for (int c = 0; c < 3; c++)
    {
      const double first = a[r] * b[4 * c], second = a[4 + r] * b[4 * c + 1], third = a[8 + r] * b[4 * c + 2];
      const double pair = first + second;
      out[4 * c + r] = pair + third;
    }
    const double first = a[r] * b[12], second = a[4 + r] * b[13], third = a[8 + r] * b[14];
    const double pair = first + second, rotated = pair + third;
    out[12 + r] = rotated + a[12 + r];
  }
}

static LinkPoses Forward(const KinematicTree& tree, const std::vector<double>& q, int64_t num,
                         const Isometry3* base, const std::vector<double>& limits)
{
  const int64_t L = tree.NumLinks(), J = tree.NumJoints();
  LinkPoses out;
  out.link_poses.assign(static_cast<size_t>(num * L) * 16, 0.0);
  out.status.assign(static_cast<size_t>(num), 0);
  for (int64_t b = 0; b < num; b++)
  {
    const double* values = q.data() + b * J;
    uint8_t bits = 0;
    if (!limits.empty())
      for (int64_t j = 0; j < J; j++)
        if (values[j] < limits[static_cast<size_t>(2 * j)] || values[j] > limits[static_cast<size_t>(2 * j + 1)])
          bits |= VGT_HIP_FK_OUTSIDE_LIMITS;
    for (int64_t i = 0; i < L; i++)
    {
      const KinematicLink& link = tree.Links()[static_cast<size_t>(i)];
      double* pose = out.link_poses.data() + (b * L + i) * 16;
      double frame[16] = {};
      if (link.parent >= 0)
        Product(out.link_poses.data() + (b * L + link.parent) * 16, link.origin.m.data(), frame);
      else if (base)
        Product(base->m.data(), link.origin.m.data(), frame);
      else
        for (int e = 0; e < 16; e++) frame[e] = link.origin.m[static_cast<size_t>(e)];
      for (int e = 0; e < 16; e++) pose[e] = frame[e];
      if (link.joint_type != VGT_HIP_JOINT_FIXED)
      {
        const double value = values[link.joint_index];
        const double x = link.axis[0], y = link.axis[1], z = link.axis[2];
        bool computable = std::isfinite(value);
        if (link.joint_type == VGT_HIP_JOINT_REVOLUTE && !(std::fabs(value) <= 0x1p+20)) computable = false;
        if (!computable)
        {
          bits |= VGT_HIP_FK_NOT_COMPUTABLE;
          for (int e = 0; e < 16; e++) pose[e] = kNaN;
        }
        else if (link.joint_type == VGT_HIP_JOINT_REVOLUTE)
        {
          double s, c;
          SinCos(value, s, c);
          const double v = 1.0 - c;
          const double xx = x * x, xy = x * y, xz = x * z, yy = y * y, yz = y * z, zz = z * z;
          const double xs = x * s, ys = y * s, zs = z * s;
          double rotation[16] = {};
          rotation[0] = c + xx * v;
          rotation[4] = xy * v - zs;
          rotation[8] = xz * v + ys;
          rotation[1] = xy * v + zs;
          rotation[5] = c + yy * v;
          rotation[9] = yz * v - xs;
          rotation[2] = xz * v - ys;
          rotation[6] = yz * v + xs;
          rotation[10] = c + zz * v;
          double turned[16] = {};
          Product(frame, rotation, turned);
          for (int c3 = 0; c3 < 3; c3++)
            for (int r = 0; r < 3; r++) pose[4 * c3 + r] = turned[4 * c3 + r];
        }
        else
        {
          double step[16] = {};
          step[12] = x * value;
          step[13] = y * value;
          step[14] = z * value;
          double moved[16] = {};
          Product(frame, step, moved);
          for (int r = 0; r < 3; r++) pose[12 + r] = moved[12 + r];
        }
      }
      pose[3] = pose[7] = pose[11] = 0.0;
      pose[15] = 1.0;
    }
    out.status[static_cast<size_t>(b)] = bits;
  }
  return out;
}

// adds the terms of sphere s (on link k in [0, L)) with gradient g to acc [J]; weight null: the worst-sphere form
static void Walk(const KinematicTree& tree, const double* poses_b, const SphereModel& model, int64_t s, int64_t k,
                 const double* g, const double* weight, double* acc)
{
  const double* m = poses_b + k * 16;
  const std::array<double, 4>& centre = model.xyzr[static_cast<size_t>(s)];
  double p[3];
  for (int r = 0; r < 3; r++)
  {
    const double first = m[r] * centre[0], second = m[4 + r] * centre[1], third = m[8 + r] * centre[2];
    const double pair = first + second, rotated = pair + third;
    p[r] = rotated + m[12 + r];
  }
  for (int64_t i = k; i >= 0; i = tree.Links()[static_cast<size_t>(i)].parent)
  {
    const KinematicLink& link = tree.Links()[static_cast<size_t>(i)];
    if (link.joint_type == VGT_HIP_JOINT_FIXED) continue;
    m = poses_b + i * 16;
    double a[3];
    for (int r = 0; r < 3; r++)
    {
      const double first = m[r] * link.axis[0], second = m[4 + r] * link.axis[1], third = m[8 + r] * link.axis[2];
      const double pair = first + second;
      a[r] = pair + third;
    }
    double term;
    if (link.joint_type == VGT_HIP_JOINT_REVOLUTE)
    {
      const double d0 = p[0] - m[12], d1 = p[1] - m[13], d2 = p[2] - m[14];
      const double u0a = a[1] * d2, u0b = a[2] * d1, u1a = a[2] * d0, u1b = a[0] * d2, u2a = a[0] * d1, u2b = a[1] * d0;
      const double u0 = u0a - u0b, u1 = u1a - u1b, u2 = u2a - u2b;
      const double first = g[0] * u0, second = g[1] * u1, third = g[2] * u2, pair = first + second;
      term = pair + third;
    }
    else
    {
      const double first = g[0] * a[0], second = g[1] * a[1], third = g[2] * a[2], pair = first + second;
      term = pair + third;
    }
    const double scaled = weight ? *weight * term : term;
    acc[link.joint_index] = acc[link.joint_index] + scaled;
  }
}

static std::vector<double> Gradient(const KinematicTree& tree, const std::vector<double>& poses, const SphereModel& model,
                                    const std::vector<int32_t>* min_sphere, const std::vector<double>* min_gradient,
                                    const std::vector<double>* weight, const std::vector<double>* gradient)
{
  const int64_t L = tree.NumLinks(), J = tree.NumJoints(), S = static_cast<int64_t>(model.link.size());
  const int64_t num = static_cast<int64_t>(poses.size()) / (L * 16);
  std::vector<double> out(static_cast<size_t>(num * J), 0.0);
  for (int64_t b = 0; b < num; b++)
  {
    double* acc = out.data() + b * J;
    const double* poses_b = poses.data() + b * L * 16;
    if (min_sphere)
    {
      const int64_t s = (*min_sphere)[static_cast<size_t>(b)];
      const int64_t k = s >= 0 && s < S ? model.link[static_cast<size_t>(s)] : -1;
      if (k < 0 || k >= L)
        for (int64_t j = 0; j < J; j++) acc[j] = kNaN;
      else
        Walk(tree, poses_b, model, s, k, min_gradient->data() + 3 * b, nullptr, acc);
    }
    else
      for (int64_t s = 0; s < S; s++)
      {
        const double* w = weight->data() + b * S + s;
        const int64_t k = model.link[static_cast<size_t>(s)];
        if (*w == 0.0 || k < 0 || k >= L) continue;
        Walk(tree, poses_b, model, s, k, gradient->data() + 3 * (b * S + s), w, acc);
      }
  }
  return out;
}
}  // namespace restated

static KinematicLink Link(int32_t parent, int32_t type, int32_t index, double ax, double ay, double az,
                          const Isometry3& origin)
{
  KinematicLink link;
  link.parent = parent;
  link.joint_type = type;
  link.joint_index = index;
  link.axis = {{ax, ay, az}};
  link.origin = origin;
  return link;
}

// a lift along z, a shoulder turning about z one unit out along x, a fixed hand one unit further along x, and a second
// hand on the lift (a branch)
static KinematicTree SmallTree()
{
  return KinematicTree({Link(-1, VGT_HIP_JOINT_PRISMATIC, 0, 0, 0, 1, Isometry3::Identity()),
                        Link(0, VGT_HIP_JOINT_REVOLUTE, 1, 0, 0, 1, Isometry3::Translation(1, 0, 0)),
                        Link(1, VGT_HIP_JOINT_FIXED, 0, 0, 0, 1, Isometry3::Translation(1, 0, 0)),
                        Link(0, VGT_HIP_JOINT_FIXED, 0, 0, 0, 1, Isometry3::Translation(0, 2, 0))},
                       2);
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

static int RunNoDevice()
{
  const double nan = std::numeric_limits<double>::quiet_NaN(), pi = 3.14159265358979323846;
  const KinematicTree tree = SmallTree();
  CHECK(tree.NumLinks() == 4 && tree.NumJoints() == 2 && tree.HipDevice() == 0);

  // the restatement against answers derived by hand
  {
    double s, c;
    restated::SinCos(0.0, s, c);
    CHECK(s == 0.0 && !std::signbit(s) && c == 1.0);
    restated::SinCos(pi / 2, s, c);
    CHECK(s == 1.0 && std::fabs(c - 6.123233995736766e-17) < 1e-30);  // (cos of the double next to pi / 2)
    restated::SinCos(1.0, s, c);
    CHECK(std::fabs(s - std::sin(1.0)) <= 0x1p-51 && std::fabs(c - std::cos(1.0)) <= 0x1p-51);
    // lift 0.5, shoulder a quarter turn: the hand is one unit along +y from the shoulder
    const std::vector<double> q = {0.5, pi / 2, 0.0, 0.0, 0.25, nan, 3.0, 0.0};
    const LinkPoses got = restated::Forward(tree, q, 4, nullptr, {-1.0, 1.0, -2.0, 2.0});
    const double* hand = got.link_poses.data() + 2 * 16;
    CHECK(hand[12] == 1.0 + 6.123233995736766e-17 && hand[13] == 1.0 && hand[14] == 0.5);
    CHECK(hand[3] == 0.0 && hand[7] == 0.0 && hand[11] == 0.0 && hand[15] == 1.0);
    CHECK(std::fabs(hand[0]) < 1e-16 && hand[1] == 1.0 && hand[4] == -1.0 && hand[10] == 1.0);
    const double* other = got.link_poses.data() + 3 * 16;
    CHECK(other[12] == 0.0 && other[13] == 2.0 && other[14] == 0.5 && other[0] == 1.0);
    // zero joints: the poses are the products of the origins, bit for bit
    const double* rest = got.link_poses.data() + (4 + 2) * 16;
    CHECK(rest[12] == 2.0 && rest[13] == 0.0 && rest[14] == 0.0 && rest[0] == 1.0 && rest[5] == 1.0 && rest[1] == 0.0);
    // a NaN shoulder: the shoulder and the hand are NaN, the lift and the other hand are not
    const double* third = got.link_poses.data() + 2 * 4 * 16;
    CHECK(third[14] == 0.25 && std::isnan(third[16]) && std::isnan(third[16 + 14]) && std::isnan(third[32 + 12]));
    CHECK(third[16 + 15] == 1.0 && third[48 + 13] == 2.0 && third[48 + 14] == 0.25);
    CHECK(got.status == (std::vector<uint8_t>{0, 0, VGT_HIP_FK_NOT_COMPUTABLE, VGT_HIP_FK_OUTSIDE_LIMITS}));
    // under a base transform
    const Isometry3 base = Isometry3::Translation(10, 20, 30);
    const LinkPoses moved = restated::Forward(tree, q, 1, &base, {});
    CHECK(moved.link_poses[2 * 16 + 13] == 21.0 && moved.link_poses[2 * 16 + 14] == 30.5);

    // the gradient: a sphere at the hand's origin, pushed along +x, in the rest pose: turning the shoulder moves the
    // hand along +y (no change along x), lifting moves it along z; pushed along +y: the lever arm is 1
    SphereModel model;
    model.link = {2, 3};
    model.xyzr = {{{0.0, 0.0, 0.0, 0.1}}, {{0.0, 0.0, 0.0, 0.1}}};
    const std::vector<double> rest_q = {0.0, 0.0};
    const LinkPoses at_rest = restated::Forward(tree, rest_q, 1, nullptr, {});
    const std::vector<int32_t> worst = {0};
    std::vector<double> push = {1.0, 0.0, 0.0};
    std::vector<double> gradient = restated::Gradient(tree, at_rest.link_poses, model, &worst, &push, nullptr, nullptr);
    CHECK(gradient == (std::vector<double>{0.0, 0.0}));
    push = {0.0, 1.0, 2.0};
    gradient = restated::Gradient(tree, at_rest.link_poses, model, &worst, &push, nullptr, nullptr);
    CHECK(gradient == (std::vector<double>{2.0, 1.0}));
    // the summed form: sphere 1 sits on the lift's branch and does not see the shoulder
    const std::vector<double> weights = {0.5, 2.0}, pushes = {0.0, 1.0, 2.0, 0.0, 0.0, 1.0};
    gradient = restated::Gradient(tree, at_rest.link_poses, model, nullptr, nullptr, &weights, &pushes);
    CHECK(gradient == (std::vector<double>{0.5 * 2.0 + 2.0 * 1.0, 0.5}));
    const std::vector<int32_t> nobody = {-1};
    gradient = restated::Gradient(tree, at_rest.link_poses, model, &nobody, &push, nullptr, nullptr);
    CHECK(std::isnan(gradient[0]) && std::isnan(gradient[1]));
  }

  // argument errors of the layer, raised before a device is asked for
  const Isometry3 eye = Isometry3::Identity();
  CHECK(ThrowsInvalidArgument([&] { KinematicTree({}, 0); }, "at least one link"));
  CHECK(ThrowsInvalidArgument([&] { KinematicTree({Link(-1, 0, 0, 0, 0, 1, eye)}, -1); }, "negative"));
  CHECK(ThrowsInvalidArgument([&] { KinematicTree({Link(0, 0, 0, 0, 0, 1, eye)}, 0); }, "link 0: parent 0 is not below 0"));
  CHECK(ThrowsInvalidArgument(
      [&] { KinematicTree({Link(-1, 0, 0, 0, 0, 1, eye), Link(-1, 0, 0, 0, 0, 1, eye), Link(7, 0, 0, 0, 0, 1, eye)}, 0); },
      "link 2: parent 7 is not below 2"));
  CHECK(ThrowsInvalidArgument([&] { KinematicTree({Link(-2, 0, 0, 0, 0, 1, eye)}, 0); }, "link 0: parent -2"));
  CHECK(ThrowsInvalidArgument([&] { KinematicTree({Link(-1, 3, 0, 0, 0, 1, eye)}, 1); }, "link 0: joint type 3"));
  CHECK(ThrowsInvalidArgument([&] { KinematicTree({Link(-1, 1, 0, 0, 0, 1, eye)}, 0); }, "link 0: joint index 0 is not in [0, 0)"));
  CHECK(ThrowsInvalidArgument([&] { KinematicTree({Link(-1, 0, 9, 0, 0, 1, eye), Link(0, 2, 2, 0, 0, 1, eye)}, 2); },
                              "link 1: joint index 2 is not in [0, 2)"));
  CHECK(ThrowsInvalidArgument([&] { ComputeLinkPoses(tree, {0.0, 0.0}, -1); }, "negative"));
  CHECK(ThrowsInvalidArgument([&] { ComputeLinkPoses(tree, {0.0, 0.0, 0.0}, 1); }, "one value per configuration and joint"));
  CHECK(ThrowsInvalidArgument([&] { ComputeLinkPoses(tree, {0.0, 0.0}, 1, nullptr, {0.0, 1.0}); }, "joint_limits"));
  {
    SphereModel model;
    model.link = {2};
    model.xyzr = {{{0.0, 0.0, 0.0, 0.1}}};
    SphereModelChecks checks;
    checks.min_sphere = {0};
    checks.min_gradient = {1.0, 0.0, 0.0};
    const std::vector<double> poses(4 * 16, 0.0);
    CHECK(ThrowsInvalidArgument([&] { ClearanceJointGradient(tree, std::vector<double>(63, 0.0), model, checks); },
                                "per configuration"));
    checks.min_gradient.pop_back();
    CHECK(ThrowsInvalidArgument([&] { ClearanceJointGradient(tree, poses, model, checks); }, "belong to"));
    CHECK(ThrowsInvalidArgument([&] { ClearanceJointGradient(tree, poses, model, {1.0}, {0.0, 0.0}); }, "belong to"));
    SphereModel bad = model;
    bad.link.push_back(0);
    CHECK(ThrowsInvalidArgument([&] { ClearanceJointGradient(tree, poses, bad, checks); }, "one link"));

    SignedDistanceField sdf;
    sdf.grid = DenseGrid(eye, "f", 1.0, 4, 4, 4, 1.0f);
    CHECK(ThrowsInvalidArgument([&] { CheckSphereModel(SignedDistanceField(), model, tree, {0.0, 0.0}); }, "initialized"));
    CHECK(ThrowsInvalidArgument([&] { CheckSphereModel(sdf, model, tree, {0.0, 0.0, 0.0}); }, "one value per"));
    bad = model;
    bad.link[0] = 4;
    CHECK(ThrowsInvalidArgument([&] { CheckSphereModel(sdf, bad, tree, {0.0, 0.0}); }, "sphere 0: link 4"));
    bad = model;
    bad.xyzr[0][3] = nan;
    CHECK(ThrowsInvalidArgument([&] { CheckSphereModel(sdf, bad, tree, {0.0, 0.0}); }, "sphere 0: the radius"));
    JointSphereModelOptions options;
    options.minimum_clearance = nan;
    CHECK(ThrowsInvalidArgument([&] { CheckSphereModel(sdf, model, tree, {0.0, 0.0}, options); }, "minimum_clearance"));
    options = JointSphereModelOptions();
    options.joint_limits = {0.0};
    CHECK(ThrowsInvalidArgument([&] { CheckSphereModel(sdf, model, tree, {0.0, 0.0}, options); }, "joint_limits"));

    // nothing to compute: no device is needed
    const LinkPoses none = ComputeLinkPoses(tree, {}, 0);
    CHECK(none.link_poses.empty() && none.status.empty());
    checks.min_sphere.clear();
    checks.min_gradient.clear();
    CHECK(ClearanceJointGradient(tree, {}, model, checks).empty());
    CHECK(ClearanceJointGradient(tree, {}, model, std::vector<double>(), std::vector<double>()).empty());
    CHECK(ClearanceJointGradient(tree, poses, SphereModel(), std::vector<double>(), std::vector<double>()) ==
          (std::vector<double>{0.0, 0.0}));
    options = JointSphereModelOptions();
    options.joint_gradient = options.per_sphere = true;
    const JointSphereModelChecks empty = CheckSphereModel(sdf, model, tree, {}, options);
    CHECK(empty.checks.status.empty() && empty.fk_status.empty() && empty.joint_gradient.empty());
  }

  // the C ABI's own errors, before the context is looked at
  {
    double memory[64] = {};
    vgt_hip_ctx* stand_in = reinterpret_cast<vgt_hip_ctx*>(memory);
    const int32_t parent[2] = {-1, 1}, kind[2] = {0, 0}, index[2] = {0, 0};
    const double axis[6] = {0, 0, 1, 0, 0, 1};
    vgt_hip_kinematics* handle = reinterpret_cast<vgt_hip_kinematics*>(memory);
    CHECK(vgt_hip_kinematics_create(stand_in, 2, 0, parent, kind, index, axis, memory, &handle) ==
          VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "link 1: parent 1 is not below 1") != nullptr && handle == nullptr);
    CHECK(vgt_hip_kinematics_create(nullptr, 2, 0, parent, kind, index, axis, memory, &handle) ==
          VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "null") != nullptr);
    vgt_hip_kinematics_destroy(nullptr);
    const vgt_hip_kinematics* fake = reinterpret_cast<const vgt_hip_kinematics*>(memory);
    CHECK(vgt_hip_forward_kinematics(stand_in, fake, memory, -1, nullptr, nullptr, memory, nullptr) ==
          VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "negative") != nullptr);
    CHECK(vgt_hip_forward_kinematics(stand_in, fake, memory, 0, nullptr, nullptr, memory, nullptr) == VGT_HIP_OK);
    CHECK(vgt_hip_clearance_joint_gradient(stand_in, fake, memory, 2, memory, parent, 1, nullptr, nullptr, nullptr,
                                           nullptr, memory) == VGT_HIP_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(vgt_hip_last_error(), "exactly one pair") != nullptr);
    CHECK(vgt_hip_kinematics_lds_links() >= 1);
  }
  return g_failures;
}

static int RunDevice()
{
  // the hand-derived tree through the layer
  {
    const KinematicTree tree = SmallTree();
    const double pi = 3.14159265358979323846;
    const std::vector<double> q = {0.5, pi / 2, 0.0, 0.0, 0.25, std::numeric_limits<double>::quiet_NaN(), 3.0, 0.0};
    const std::vector<double> limits = {-1.0, 1.0, -2.0, 2.0};
    const LinkPoses got = ComputeLinkPoses(tree, q, 4, nullptr, limits);
    const LinkPoses want = restated::Forward(tree, q, 4, nullptr, limits);
    CHECK(SameDoubles(got.link_poses, want.link_poses) && SameBytes(got.status, want.status));
    CHECK(got.link_poses[2 * 16 + 13] == 1.0 && got.link_poses[2 * 16 + 14] == 0.5);
    const KinematicTree copy = tree;  // (copies share the device tree)
    CHECK(copy.DeviceTree() == tree.DeviceTree() && vgt_hip_kinematics_num_links(tree.DeviceTree()) == 4);
  }
  // an arm on a base with a branch, 11 links, 6 joints (one read by two links), 150 configurations, a rolling field
  {
    uint64_t state = 4711;
    auto next = [&]() {  // uniform in [0, 1)
      state = state * 6364136223846793005ull + 1442695040888963407ull;
      return static_cast<double>(state >> 11) * (1.0 / 9007199254740992.0);
    };
    auto origin = [&]() {
      const double angle = next() * 6.0;
      return Isometry3::FromQuaternion(std::cos(angle), std::sin(angle) * 0.6, 0.0, std::sin(angle) * 0.8,
                                       next() * 0.3 - 0.1, next() * 0.3 - 0.1, next() * 0.3);
    };
    std::vector<KinematicLink> links;
    const int32_t parents[11] = {-1, 0, 1, 2, 3, 4, 2, 6, 7, 1, 5};
    const int32_t kinds[11] = {2, 1, 1, 1, 0, 1, 1, 2, 0, 1, 2};
    const int32_t columns[11] = {0, 1, 2, 3, 0, 4, 3, 5, 0, 4, 5};
    for (int i = 0; i < 11; i++)
      links.push_back(Link(parents[i], kinds[i], columns[i], next() - 0.5, next() - 0.5, next() + 0.2, origin()));
    const KinematicTree tree(links, 6);
    const int64_t num = 150;
    std::vector<double> q;
    for (int64_t i = 0; i < num * 6; i++) q.push_back(next() * 6.0 - 3.0);
    q[6 * 3 + 2] = std::numeric_limits<double>::quiet_NaN();
    q[6 * 5 + 0] = std::numeric_limits<double>::infinity();
    q[6 * 7 + 1] = 1048576.0;
    q[6 * 8 + 1] = std::nextafter(1048576.0, 2e6);
    for (int j = 0; j < 6; j++) q[static_cast<size_t>(6 * 9 + j)] = 0.0;
    std::vector<double> limits;
    for (int j = 0; j < 6; j++)
    {
      limits.push_back(-2.5);
      limits.push_back(2.0);
    }
    const Isometry3 base = Isometry3::FromQuaternion(std::cos(0.3), 0.0, std::sin(0.3), 0.0, 0.6, 0.5, 0.4);
    const LinkPoses got = ComputeLinkPoses(tree, q, num, &base, limits);
    const LinkPoses want = restated::Forward(tree, q, num, &base, limits);
    CHECK(SameDoubles(got.link_poses, want.link_poses) && SameBytes(got.status, want.status));
    const LinkPoses plain = ComputeLinkPoses(tree, q, num);
    const LinkPoses plain_want = restated::Forward(tree, q, num, nullptr, {});
    CHECK(SameDoubles(plain.link_poses, plain_want.link_poses) && SameBytes(plain.status, plain_want.status));
    int not_computable = 0, outside = 0;
    for (uint8_t bits : got.status)
    {
      not_computable += (bits & VGT_HIP_FK_NOT_COMPUTABLE) ? 1 : 0;
      outside += (bits & VGT_HIP_FK_OUTSIDE_LIMITS) ? 1 : 0;
    }
    CHECK(not_computable == 3 && outside > 10 && outside < 150);

    SignedDistanceField sdf;
    sdf.grid = DenseGrid(Isometry3::Identity(), "f", 0.125, 11, 9, 13, 0.0f);
    for (int64_t x = 0; x < 11; x++)
      for (int64_t y = 0; y < 9; y++)
        for (int64_t z = 0; z < 13; z++)
          sdf.grid.SetIndex(x, y, z, static_cast<float>(0.3 * std::sin(0.7 * x) + 0.25 * std::cos(0.9 * y) - 0.1 * z + 0.4));
    SphereModel model;
    for (int s = 0; s < 23; s++)
    {
      model.link.push_back(static_cast<int32_t>(next() * 11.0) % 11);
      model.xyzr.push_back({{next() * 0.2 - 0.1, next() * 0.2 - 0.1, next() * 0.2 - 0.1, s % 4 == 0 ? 0.0 : next() * 0.05}});
    }
    // the two-step route, each step against the restatement; then the chained call against the two steps
    SphereModelOptions step_options;
    step_options.minimum_clearance = 0.05;
    step_options.per_sphere = true;
    const SphereModelChecks checks = CheckSphereModel(sdf, model, got.link_poses, 11, step_options);
    const std::vector<double> worst = ClearanceJointGradient(tree, got.link_poses, model, checks);
    CHECK(SameDoubles(worst, restated::Gradient(tree, want.link_poses, model, &checks.min_sphere, &checks.min_gradient,
                                                nullptr, nullptr)));
    std::vector<double> weights;
    for (size_t i = 0; i < checks.sphere_clearance.size(); i++)
      weights.push_back(checks.sphere_clearance[i] < 0.3 ? 0.3 - checks.sphere_clearance[i] : 0.0);  // (NaN: 0)
    const std::vector<double> summed = ClearanceJointGradient(tree, got.link_poses, model, weights, checks.sphere_gradient);
    CHECK(SameDoubles(summed, restated::Gradient(tree, want.link_poses, model, nullptr, nullptr, &weights,
                                                 &checks.sphere_gradient)));
    int finite = 0;
    for (double v : summed) finite += std::isfinite(v) && v != 0.0 ? 1 : 0;
    CHECK(finite > 100);

    JointSphereModelOptions options;
    options.minimum_clearance = 0.05;
    options.per_sphere = true;
    options.joint_gradient = true;
    options.has_world_from_base = true;
    options.world_from_base = base;
    options.joint_limits = limits;
    const JointSphereModelChecks chained = CheckSphereModel(sdf, model, tree, q, options);
    CHECK(SameBytes(chained.checks.status, checks.status) && SameBytes(chained.checks.min_sphere, checks.min_sphere));
    CHECK(SameBytes(chained.checks.num_below, checks.num_below) && SameBytes(chained.checks.num_outside, checks.num_outside));
    CHECK(SameDoubles(chained.checks.min_clearance, checks.min_clearance));
    CHECK(SameDoubles(chained.checks.min_gradient, checks.min_gradient));
    CHECK(SameDoubles(chained.checks.sphere_clearance, checks.sphere_clearance));
    CHECK(SameDoubles(chained.checks.sphere_gradient, checks.sphere_gradient));
    CHECK(SameBytes(chained.fk_status, got.status) && SameDoubles(chained.joint_gradient, worst));
    options.per_sphere = options.joint_gradient = false;
    const JointSphereModelChecks brief = CheckSphereModel(sdf, model, tree, q, options);
    CHECK(brief.checks.sphere_clearance.empty() && brief.joint_gradient.empty());
    CHECK(SameBytes(brief.checks.status, checks.status) && SameBytes(brief.fk_status, got.status));
    int statuses[3] = {0, 0, 0};
    for (uint8_t v : checks.status) statuses[v]++;
    CHECK(statuses[0] + statuses[1] > 50 && statuses[1] > 0);

    // The same field on an origin turned by 0.7 about (0.3, -0.5, 0.8) -- an axis that is none of x, y, z -- and shifted,
    // the base moved with it: the chained call against the two steps under that grid (test_body_host.cc holds
    // CheckSphereModel on given poses under a turned grid to its restatement).
    const double s = std::sin(0.35) / std::sqrt(0.3 * 0.3 + 0.5 * 0.5 + 0.8 * 0.8);
    const Isometry3 turn = Isometry3::FromQuaternion(std::cos(0.35), 0.3 * s, -0.5 * s, 0.8 * s, 0.4, -0.2, 0.05);
    SignedDistanceField turned_sdf;
    turned_sdf.grid = DenseGrid(turn, "f", 0.125, 11, 9, 13, 0.0f);
    for (int64_t x = 0; x < 11; x++)
      for (int64_t y = 0; y < 9; y++)
        for (int64_t z = 0; z < 13; z++) turned_sdf.grid.SetIndex(x, y, z, sdf.grid.GetIndexImmutable(x, y, z));
    const Isometry3 turned_base = turn * base;
    const LinkPoses turned_poses = ComputeLinkPoses(tree, q, num, &turned_base, limits);
    const SphereModelChecks turned_checks = CheckSphereModel(turned_sdf, model, turned_poses.link_poses, 11, step_options);
    const std::vector<double> turned_worst = ClearanceJointGradient(tree, turned_poses.link_poses, model, turned_checks);
    options.per_sphere = options.joint_gradient = true;
    options.world_from_base = turned_base;
    const JointSphereModelChecks turned_chained = CheckSphereModel(turned_sdf, model, tree, q, options);
    CHECK(SameBytes(turned_chained.checks.status, turned_checks.status));
    CHECK(SameBytes(turned_chained.checks.min_sphere, turned_checks.min_sphere));
    CHECK(SameBytes(turned_chained.checks.num_below, turned_checks.num_below));
    CHECK(SameBytes(turned_chained.checks.num_outside, turned_checks.num_outside));
    CHECK(SameDoubles(turned_chained.checks.min_clearance, turned_checks.min_clearance));
    CHECK(SameDoubles(turned_chained.checks.min_gradient, turned_checks.min_gradient));
    CHECK(SameDoubles(turned_chained.checks.sphere_clearance, turned_checks.sphere_clearance));
    CHECK(SameDoubles(turned_chained.checks.sphere_gradient, turned_checks.sphere_gradient));
    CHECK(SameBytes(turned_chained.fk_status, turned_poses.status) && SameDoubles(turned_chained.joint_gradient, turned_worst));
    // (the scene is the same one: most configurations keep their status, and the gradients are other vectors)
    int same_status = 0, other_gradient = 0;
    for (size_t b = 0; b < checks.status.size(); b++)
    {
      same_status += turned_checks.status[b] == checks.status[b] ? 1 : 0;
      other_gradient += std::fabs(turned_checks.min_gradient[3 * b] - checks.min_gradient[3 * b]) > 1e-3 ? 1 : 0;
    }
    CHECK(same_status > 135 && other_gradient > 50);
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
