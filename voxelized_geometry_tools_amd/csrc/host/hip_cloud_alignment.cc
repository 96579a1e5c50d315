// AlignPointCloud of include/vgt_hip/cloud_alignment.hpp on the C ABI (vgt_hip_align_points).
#include "../../../include/vgt_hip/cloud_alignment.hpp"
#include "host_internal.hpp"

#include <array>
#include <cmath>

namespace vgt_hip
{
CloudAlignment AlignPointCloud(const SignedDistanceField& sdf, const std::vector<float>& points,
                               const std::vector<Isometry3>& initial_poses, const CloudAlignmentOptions& options)
{
  const DenseGrid& g = sdf.grid;
  if (!g.IsInitialized()) throw std::invalid_argument("Grid must be initialized");
  if (points.size() % 3 != 0) throw std::invalid_argument("points must hold three floats per point");
  if (!options.pivot.empty() && options.pivot.size() != 3)
    throw std::invalid_argument("the pivot must hold three doubles (or none: the centre of the grid)");
  // (what the C ABI would refuse, refused before a device is asked for)
  if (points.empty() || initial_poses.empty())
    throw std::invalid_argument("cloud alignment needs a grid, a cloud and poses that are not empty");
  if (options.max_iterations < 0 || options.max_iterations > 10000)
    throw std::invalid_argument("max_iterations must be in [0, 10000]");
  if (options.min_points < 6) throw std::invalid_argument("min_points must be at least 6");
  if (!(options.damping >= 0.0) || !std::isfinite(options.damping))
    throw std::invalid_argument("damping must be finite and not negative");
  if (!(options.max_residual > 0.0)) throw std::invalid_argument("max_residual must be positive (or +infinity)");
  if (!std::isfinite(options.target_distance)) throw std::invalid_argument("target_distance must be finite");
  if (!(options.translation_tolerance >= 0.0) || !(options.rotation_tolerance >= 0.0))
    throw std::invalid_argument("the tolerances must not be negative or NaN");
  for (const double p : options.pivot)
    if (!std::isfinite(p)) throw std::invalid_argument("the pivot must be finite");

  std::array<double, 9> rotation{};
  for (int row = 0; row < 3; row++)
    for (int col = 0; col < 3; col++) rotation[static_cast<size_t>(row * 3 + col)] = g.OriginTransform()(row, col);
  double pivot[3];
  if (options.pivot.empty())
  {
    const double centre[3] = {0.5 * g.GridXSize(), 0.5 * g.GridYSize(), 0.5 * g.GridZSize()};
    const Isometry3& o = g.OriginTransform();
    for (int r = 0; r < 3; r++) pivot[r] = ((o(r, 0) * centre[0] + o(r, 1) * centre[1]) + o(r, 2) * centre[2]) + o(r, 3);
  }
  else
  {
    for (int r = 0; r < 3; r++) pivot[r] = options.pivot[static_cast<size_t>(r)];
  }

  static_assert(sizeof(Isometry3) == 16 * sizeof(double), "the poses are passed as packed doubles");
  const size_t b = initial_poses.size();
  CloudAlignment out;
  out.poses.resize(b);
  out.status.resize(b);
  out.num_used.resize(b);
  out.num_outside.resize(b);
  out.num_rejected.resize(b);
  out.sum_squared.resize(b);
  out.evaluations.resize(b);
  out.normal_equations.resize(b * 27);
  out.last_step.resize(b * 6);
  const int rc = vgt_hip_align_points(
      detail::SharedSdfContext(options.hip_device), g.GetImmutableRawData().data(), g.NumXVoxels(), g.NumYVoxels(),
      g.NumZVoxels(), g.Resolution(), g.InverseOriginTransform().m.data(), rotation.data(), points.data(),
      static_cast<int64_t>(points.size() / 3), initial_poses[0].m.data(), static_cast<int64_t>(b), pivot,
      options.max_iterations, options.min_points, options.damping, options.max_residual, options.target_distance,
      options.translation_tolerance, options.rotation_tolerance, out.poses[0].m.data(), out.status.data(),
      out.num_used.data(), out.num_outside.data(), out.num_rejected.data(), out.sum_squared.data(),
      out.evaluations.data(), out.normal_equations.data(), out.last_step.data());
  if (rc != VGT_HIP_OK) detail::ThrowForCode(rc, vgt_hip_last_error());
  return out;
}

CloudAlignment AlignPointCloud(const SignedDistanceField& sdf, const PointCloudWrapper& cloud,
                               const std::vector<Isometry3>& initial_poses, const CloudAlignmentOptions& options)
{
  const int64_t n = cloud.Size();
  if (n < 0) throw std::invalid_argument("the cloud's size must not be negative");
  std::vector<float> points(static_cast<size_t>(n) * 3);
  for (int64_t i = 0; i < n; i++) cloud.CopyPointLocationIntoFloatPtr(i, points.data() + 3 * i);
  return AlignPointCloud(sdf, points, initial_poses, options);
}
}  // namespace vgt_hip
