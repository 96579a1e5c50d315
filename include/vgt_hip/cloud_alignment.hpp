// Cloud alignment of the C++ host layer: where is the sensor with respect to the map?  A point cloud under a batch of
// pose hypotheses against a signed distance field, each hypothesis scored and refined by damped Gauss-Newton steps on the
// device (vgt_hip_align_points of vgt_hip.h, which states the definition and every output).  With max_iterations = 0
// the hypotheses are only scored: the measurement model of a particle filter.
#pragma once

#include <cstdint>
#include <limits>
#include <vector>

#include "host_types.hpp"

namespace vgt_hip
{
struct CloudAlignmentOptions
{
  int32_t max_iterations = 10;  // 0: score only
  int32_t min_points = 6;       // fewer used points than this stop a pose as VGT_HIP_ALIGN_TOO_FEW
  double damping = 0.0;         // the diagonal of the normal equations is scaled by 1 + damping
  double max_residual = std::numeric_limits<double>::infinity();  // points with |d - target_distance| above are not used
  double target_distance = 0.0;  // the distance the cloud's points should have (half a cell inside for cell centres)
  double translation_tolerance = 0.0, rotation_tolerance = 0.0;  // a step within both stops a pose as _CONVERGED
  // The point rotations are taken about, in the poses' frame: 3 doubles, or empty for the centre of the field's grid.
  std::vector<double> pivot;
  int hip_device = 0;
};
// One entry per initial pose; normal_equations holds 27 doubles per pose (the 21 entries of H row-major over j <= k,
// then b), last_step 6 (v, omega).  The counts, sum_squared and normal_equations are those of an evaluation at `poses`.
struct CloudAlignment
{
  std::vector<Isometry3> poses;
  std::vector<uint8_t> status;  // VGT_HIP_ALIGN_CONVERGED / _ITERATION_LIMIT / _DEGENERATE / _TOO_FEW
  std::vector<int32_t> num_used, num_outside, num_rejected;
  std::vector<double> sum_squared;
  std::vector<int32_t> evaluations;
  std::vector<double> normal_equations, last_step;
};
// `points`: 3 floats per point in the sensor's frame; `initial_poses`: world_from_points hypotheses, in the frame the
// field's origin transform maps to (the field's inverse origin transform is the call's grid_from_world, its rotation
// the call's rotation).  Uses the process's shared context of `hip_device`.  Throws std::invalid_argument where the C
// ABI reports an invalid argument (and for a field without cells, points that are not a whole number of triples, or a
// pivot of another length than 0 or 3), std::runtime_error for its other errors.
CloudAlignment AlignPointCloud(const SignedDistanceField& sdf, const std::vector<float>& points,
                               const std::vector<Isometry3>& initial_poses, const CloudAlignmentOptions& options = {});
// The cloud's points as stored (its own PointCloudOriginTransform() is one more hypothesis the caller may pass).
CloudAlignment AlignPointCloud(const SignedDistanceField& sdf, const PointCloudWrapper& cloud,
                               const std::vector<Isometry3>& initial_poses, const CloudAlignmentOptions& options = {});
}  // namespace vgt_hip
