// KinematicTree, ComputeLinkPoses, ClearanceJointGradient and CheckSphereModel from joint values
// (include/vgt_hip/kinematics.hpp) on the C ABI (vgt_hip_kinematics_create, vgt_hip_forward_kinematics,
// vgt_hip_clearance_joint_gradient, vgt_hip_check_spheres_from_joints).
#include "../../../include/vgt_hip/kinematics.hpp"
#include "host_internal.hpp"

#include <cmath>
#include <limits>
#include <mutex>

namespace vgt_hip
{
struct KinematicTree::State
{
  std::vector<KinematicLink> links;
  int64_t num_joints = 0;
  int hip_device = 0;
  std::mutex mutex;
  vgt_hip_kinematics* device_tree = nullptr;

  ~State() { vgt_hip_kinematics_destroy(device_tree); }
};

KinematicTree::KinematicTree(std::vector<KinematicLink> links, int64_t num_joints, int hip_device)
{
  // (what the C ABI would refuse, refused before a device is asked for, in its words)
  if (links.empty()) throw std::invalid_argument("a kinematic tree needs at least one link");
  if (links.size() > 0x7fffffffu) throw std::invalid_argument("a kinematic tree has fewer than 2^31 links");
  if (num_joints < 0) throw std::invalid_argument("negative number of joints");
  for (size_t i = 0; i < links.size(); i++)
  {
    const KinematicLink& link = links[i];
    const std::string name = "link " + std::to_string(i) + ": ";
    if (link.parent < -1 || link.parent >= static_cast<int64_t>(i))
      throw std::invalid_argument(name + "parent " + std::to_string(link.parent) + " is not below " + std::to_string(i));
    if (link.joint_type != VGT_HIP_JOINT_FIXED && link.joint_type != VGT_HIP_JOINT_REVOLUTE &&
        link.joint_type != VGT_HIP_JOINT_PRISMATIC)
      throw std::invalid_argument(name + "joint type " + std::to_string(link.joint_type) + " is unknown");
    if (link.joint_type != VGT_HIP_JOINT_FIXED && (link.joint_index < 0 || link.joint_index >= num_joints))
      throw std::invalid_argument(name + "joint index " + std::to_string(link.joint_index) + " is not in [0, " +
                                  std::to_string(num_joints) + ")");
  }
  state_ = std::make_shared<State>();
  state_->links = std::move(links);
  state_->num_joints = num_joints;
  state_->hip_device = hip_device;
}

int64_t KinematicTree::NumLinks() const { return static_cast<int64_t>(state_->links.size()); }
int64_t KinematicTree::NumJoints() const { return state_->num_joints; }
int KinematicTree::HipDevice() const { return state_->hip_device; }
const std::vector<KinematicLink>& KinematicTree::Links() const { return state_->links; }

const vgt_hip_kinematics* KinematicTree::DeviceTree() const
{
  std::lock_guard<std::mutex> lock(state_->mutex);
  if (state_->device_tree) return state_->device_tree;
  const std::vector<KinematicLink>& links = state_->links;
  std::vector<int32_t> parent, joint_type, joint_index;
  std::vector<double> axis, origin;
  for (const KinematicLink& link : links)
  {
    parent.push_back(link.parent);
    joint_type.push_back(link.joint_type);
    joint_index.push_back(link.joint_index);
    axis.insert(axis.end(), link.axis.begin(), link.axis.end());
    origin.insert(origin.end(), link.origin.m.begin(), link.origin.m.end());
  }
  const int rc = vgt_hip_kinematics_create(detail::SharedSdfContext(state_->hip_device),
                                           static_cast<int64_t>(links.size()), state_->num_joints, parent.data(),
                                           joint_type.data(), joint_index.data(), axis.data(), origin.data(),
                                           &state_->device_tree);
  if (rc != VGT_HIP_OK) detail::ThrowForCode(rc, vgt_hip_last_error());
  return state_->device_tree;
}

namespace
{
// B for `values` doubles at `per_configuration` each
int64_t Configurations(size_t values, int64_t per_configuration, const char* what)
{
  const size_t per = static_cast<size_t>(per_configuration);
  if (per == 0 ? values != 0 : values % per != 0) throw std::invalid_argument(what);
  return per == 0 ? 0 : static_cast<int64_t>(values / per);
}

void CheckLimits(const KinematicTree& tree, const std::vector<double>& joint_limits)
{
  if (!joint_limits.empty() && joint_limits.size() != static_cast<size_t>(tree.NumJoints()) * 2)
    throw std::invalid_argument("joint_limits must hold a lower and an upper value per joint");
}

void CheckModelVectors(const SphereModel& model)
{
  if (model.link.size() != model.xyzr.size())
    throw std::invalid_argument("a sphere model holds one link and one (x, y, z, r) per sphere");
  static_assert(sizeof(std::array<double, 4>) == 4 * sizeof(double), "the spheres are passed as packed doubles");
}
}  // namespace

LinkPoses ComputeLinkPoses(const KinematicTree& tree, const std::vector<double>& joint_values, int64_t num_configurations,
                           const Isometry3* world_from_base, const std::vector<double>& joint_limits)
{
  if (num_configurations < 0) throw std::invalid_argument("negative number of configurations");
  if (joint_values.size() != static_cast<size_t>(num_configurations) * static_cast<size_t>(tree.NumJoints()))
    throw std::invalid_argument("joint_values must hold one value per configuration and joint");
  CheckLimits(tree, joint_limits);
  if (num_configurations * tree.NumLinks() > 0x7fffffffLL)
    throw std::invalid_argument("forward kinematics supports fewer than 2^31 (configuration, link) pairs");
  LinkPoses out;
  if (num_configurations == 0) return out;  // (no device is needed)
  out.link_poses.resize(static_cast<size_t>(num_configurations * tree.NumLinks()) * 16);
  out.status.resize(static_cast<size_t>(num_configurations));
  const int rc = vgt_hip_forward_kinematics(
      detail::SharedSdfContext(tree.HipDevice()), tree.DeviceTree(), joint_values.data(), num_configurations,
      world_from_base ? world_from_base->m.data() : nullptr, joint_limits.empty() ? nullptr : joint_limits.data(),
      out.link_poses.data(), out.status.data());
  if (rc != VGT_HIP_OK) detail::ThrowForCode(rc, vgt_hip_last_error());
  return out;
}

namespace
{
std::vector<double> JointGradient(const KinematicTree& tree, const std::vector<double>& link_poses,
                                  const SphereModel& model, const std::vector<int32_t>* min_sphere,
                                  const std::vector<double>* min_gradient, const std::vector<double>* sphere_weight,
                                  const std::vector<double>* sphere_gradient)
{
  CheckModelVectors(model);
  const int64_t b = Configurations(link_poses.size(), tree.NumLinks() * 16,
                                   "link_poses must hold the tree's links * 16 doubles per configuration");
  const size_t nb = static_cast<size_t>(b), ns = model.link.size();
  if (min_sphere ? (min_sphere->size() != nb || min_gradient->size() != nb * 3)
                 : (sphere_weight->size() != nb * ns || sphere_gradient->size() != nb * ns * 3))
    throw std::invalid_argument("the check's outputs must belong to these configurations and this model");
  if (b * static_cast<int64_t>(ns) > 0x7fffffffLL || b * tree.NumJoints() > 0x7fffffffLL)
    throw std::invalid_argument("the joint gradient supports fewer than 2^31 (configuration, sphere) and "
                                "(configuration, joint) pairs");
  std::vector<double> out(nb * static_cast<size_t>(tree.NumJoints()));
  if (out.empty()) return out;  // (no device is needed)
  const int rc = vgt_hip_clearance_joint_gradient(
      detail::SharedSdfContext(tree.HipDevice()), tree.DeviceTree(), link_poses.data(), b,
      ns ? model.xyzr[0].data() : nullptr, ns ? model.link.data() : nullptr, static_cast<int64_t>(ns),
      min_sphere ? min_sphere->data() : nullptr, min_sphere ? min_gradient->data() : nullptr,
      min_sphere ? nullptr : sphere_weight->data(), min_sphere ? nullptr : sphere_gradient->data(), out.data());
  if (rc != VGT_HIP_OK) detail::ThrowForCode(rc, vgt_hip_last_error());
  return out;
}
}  // namespace

std::vector<double> ClearanceJointGradient(const KinematicTree& tree, const std::vector<double>& link_poses,
                                           const SphereModel& model, const SphereModelChecks& checks)
{
  return JointGradient(tree, link_poses, model, &checks.min_sphere, &checks.min_gradient, nullptr, nullptr);
}

std::vector<double> ClearanceJointGradient(const KinematicTree& tree, const std::vector<double>& link_poses,
                                           const SphereModel& model, const std::vector<double>& sphere_weight,
                                           const std::vector<double>& sphere_gradient)
{
  if (model.link.empty() && model.xyzr.empty() && sphere_weight.empty() && sphere_gradient.empty())
  {
    // no spheres: nothing is summed, every entry is +0.0 (and empty vectors have no address to hand to the C ABI)
    const int64_t b = Configurations(link_poses.size(), tree.NumLinks() * 16,
                                     "link_poses must hold the tree's links * 16 doubles per configuration");
    return std::vector<double>(static_cast<size_t>(b * tree.NumJoints()), 0.0);
  }
  return JointGradient(tree, link_poses, model, nullptr, nullptr, &sphere_weight, &sphere_gradient);
}

JointSphereModelChecks CheckSphereModel(const SignedDistanceField& sdf, const SphereModel& model,
                                        const KinematicTree& tree, const std::vector<double>& joint_values,
                                        const JointSphereModelOptions& options)
{
  const DenseGrid& g = sdf.grid;
  if (!g.IsInitialized()) throw std::invalid_argument("Grid must be initialized");
  CheckModelVectors(model);
  if (std::isnan(options.minimum_clearance)) throw std::invalid_argument("minimum_clearance must not be NaN");
  const int64_t s = static_cast<int64_t>(model.link.size());
  for (int64_t i = 0; i < s; i++)
  {
    const size_t k = static_cast<size_t>(i);
    if (model.link[k] < 0 || model.link[k] >= tree.NumLinks())
      throw std::invalid_argument("sphere " + std::to_string(i) + ": link " + std::to_string(model.link[k]) +
                                  " is not in [0, num_links)");
    if (!(model.xyzr[k][3] >= 0.0))
      throw std::invalid_argument("sphere " + std::to_string(i) + ": the radius must not be negative or NaN");
  }
  CheckLimits(tree, options.joint_limits);
  int64_t b = 0;
  if (tree.NumJoints() > 0)
    b = Configurations(joint_values.size(), tree.NumJoints(), "joint_values must hold one value per configuration and joint");
  else if (!joint_values.empty())
    throw std::invalid_argument("joint_values must hold one value per configuration and joint");
  if (b * s > 0x7fffffffLL || b * tree.NumLinks() > 0x7fffffffLL || b * tree.NumJoints() > 0x7fffffffLL)
    throw std::invalid_argument("sphere-model checks support fewer than 2^31 (configuration, sphere) pairs");

  JointSphereModelChecks out;
  const size_t nb = static_cast<size_t>(b), ns = static_cast<size_t>(s);
  out.checks.status.resize(nb);
  out.checks.min_clearance.resize(nb);
  out.checks.min_sphere.resize(nb);
  out.checks.num_below.resize(nb);
  out.checks.num_outside.resize(nb);
  out.checks.min_gradient.resize(nb * 3);
  if (options.per_sphere)
  {
    out.checks.sphere_clearance.resize(nb * ns);
    out.checks.sphere_gradient.resize(nb * ns * 3);
  }
  out.fk_status.resize(nb);
  if (options.joint_gradient) out.joint_gradient.resize(nb * static_cast<size_t>(tree.NumJoints()));
  if (b == 0) return out;  // (no device is needed)

  std::array<double, 9> rotation{};
  for (int row = 0; row < 3; row++)
    for (int col = 0; col < 3; col++) rotation[static_cast<size_t>(row * 3 + col)] = g.OriginTransform()(row, col);
  const bool per_sphere = options.per_sphere && ns > 0;
  const int rc = vgt_hip_check_spheres_from_joints(
      detail::SharedSdfContext(tree.HipDevice()), g.GetImmutableRawData().data(), g.NumXVoxels(), g.NumYVoxels(),
      g.NumZVoxels(), g.Resolution(), g.InverseOriginTransform().m.data(), rotation.data(),
      s ? model.xyzr[0].data() : nullptr, s ? model.link.data() : nullptr, s, tree.DeviceTree(), joint_values.data(), b,
      options.has_world_from_base ? options.world_from_base.m.data() : nullptr,
      options.joint_limits.empty() ? nullptr : options.joint_limits.data(), options.minimum_clearance,
      options.outside_is_collision ? VGT_HIP_SPHERES_OUTSIDE_IS_COLLISION : 0u, out.checks.status.data(),
      out.checks.min_clearance.data(), out.checks.min_sphere.data(), out.checks.num_below.data(),
      out.checks.num_outside.data(), out.checks.min_gradient.data(),
      per_sphere ? out.checks.sphere_clearance.data() : nullptr, per_sphere ? out.checks.sphere_gradient.data() : nullptr,
      out.fk_status.data(), out.joint_gradient.empty() ? nullptr : out.joint_gradient.data());
  if (rc != VGT_HIP_OK) detail::ThrowForCode(rc, vgt_hip_last_error());
  return out;
}
}  // namespace vgt_hip
