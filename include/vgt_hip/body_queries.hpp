// Body queries of the C++ host layer: a robot modelled as spheres attached to links, checked against a signed distance
// field in a batch of configurations on the device (vgt_hip_check_spheres of vgt_hip.h, which states every output).
// The question a planner asks for each candidate configuration; forward kinematics stays with the caller.
#pragma once

#include <array>
#include <cstdint>
#include <vector>

#include "host_types.hpp"

namespace vgt_hip
{
// One entry per sphere: the link it is attached to, and its centre in that link's frame with its radius.
struct SphereModel
{
  std::vector<int32_t> link;
  std::vector<std::array<double, 4>> xyzr;
};
struct SphereModelOptions
{
  double minimum_clearance = 0.0;     // a sphere with clearance <= this collides
  bool outside_is_collision = false;  // a sphere that is not in the grid collides too
  bool per_sphere = false;            // also return every sphere's clearance and gradient
  int hip_device = 0;
};
// One entry per configuration; sphere_clearance [B][S] and sphere_gradient [B][S][3] are empty unless per_sphere.
struct SphereModelChecks
{
  std::vector<uint8_t> status;  // VGT_HIP_SPHERES_CLEAR / _COLLISION / _NO_VALUE
  std::vector<double> min_clearance;
  std::vector<int32_t> min_sphere, num_below, num_outside;
  std::vector<double> min_gradient;  // 3 per configuration
  std::vector<double> sphere_clearance, sphere_gradient;
};
// `link_poses`: B * num_links * 16 doubles, world_from_link column-major (the memory of a std::vector<Eigen::Isometry3d>
// per configuration), in the frame the field's origin transform maps to; the field's inverse origin transform is the
// call's grid_from_world, its rotation the call's rotation.  Uses the process's shared context of `hip_device`.  Throws
// std::invalid_argument where the C ABI reports an invalid argument (and for a field without cells, a model whose two
// vectors differ in length, or poses that are not a whole number of configurations), std::runtime_error for its other
// errors.
SphereModelChecks CheckSphereModel(const SignedDistanceField& sdf, const SphereModel& model,
                                   const std::vector<double>& link_poses, int64_t num_links,
                                   const SphereModelOptions& options = {});
}  // namespace vgt_hip
