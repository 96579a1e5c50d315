// ProjectLocationsOutOfCollision of the C++ host layer (include/vgt_hip/hip_pointcloud_voxelizer.hpp) on the field of one
// filled voxel under an origin transform that rotates and translates.
//   test_projection_host              needs a HIP device
//   test_projection_host --no-device  only the argument errors that are raised before a device is touched
#include <vgt_hip.h>
#include <vgt_hip/hip_pointcloud_voxelizer.hpp>

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
static bool ThrowsInvalidArgument(const Fn& fn)
{
  try
  {
    fn();
  }
  catch (const std::invalid_argument&)
  {
    return true;
  }
  catch (...)
  {
  }
  return false;
}

static int RunNoDevice()
{
  SignedDistanceField sdf;
  sdf.grid = DenseGrid(Isometry3::Identity(), "f", 0.1, 5, 5, 5, 0.0f);
  CHECK(ThrowsInvalidArgument([&] { ProjectLocationsOutOfCollision(sdf, {0.1, 0.2}); }));
  // the C ABI rejects these before any HIP call, and leaves its outputs alone (the field stands in for a context:
  // a non-null context pointer is not dereferenced before the other checks)
  const float* field = sdf.grid.GetImmutableRawData().data();
  vgt_hip_ctx* stand_in = reinterpret_cast<vgt_hip_ctx*>(const_cast<float*>(field));
  const double query[3] = {0.25, 0.25, 0.25};
  double position[3] = {7.0, 7.0, 7.0};
  uint8_t has_value = 9, status = 9;
  int32_t iterations = 9;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const auto call = [&](vgt_hip_ctx* ctx, int64_t nx, double resolution, double minimum_distance, double multiplier,
                        int32_t max_iterations, double* out) {
    return vgt_hip_sdf_project_out_of_collision(ctx, field, nx, 5, 5, resolution, nullptr, nullptr, query, 1,
                                                minimum_distance, multiplier, max_iterations, out, &has_value, &status,
                                                &iterations);
  };
  CHECK(call(nullptr, 5, 0.1, 0.0, 0.1, 0, position) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "null") != nullptr);
  CHECK(call(stand_in, 5, 0.1, 0.0, 0.1, 0, nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "null") != nullptr);
  CHECK(call(stand_in, 0, 0.1, 0.0, 0.1, 0, position) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "positive") != nullptr);
  CHECK(call(stand_in, 5, 0.0, 0.0, 0.1, 0, position) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "resolution") != nullptr);
  CHECK(call(stand_in, 5, 0.1, nan, 0.1, 0, position) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "minimum_distance") != nullptr);
  CHECK(call(stand_in, 5, 0.1, 0.0, 0.0, 0, position) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "stepsize_multiplier") != nullptr);
  CHECK(call(stand_in, 5, 0.1, 0.0, nan, 0, position) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(call(stand_in, 5, 0.1, 0.0, 0.1, -1, position) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "max_iterations") != nullptr);
  CHECK(position[0] == 7.0 && position[1] == 7.0 && position[2] == 7.0 && has_value == 9 && status == 9 && iterations == 9);
  return g_failures;
}

static int RunDevice()
{
  // 5^3 cells of 0.1, the centre voxel filled; the grid frame is turned about z and moved
  const double half = 0.5 * 0.6435011087932844;  // cos = 0.8, sin = 0.6
  const Isometry3 origin = Isometry3::FromQuaternion(std::cos(half), 0.0, 0.0, std::sin(half), 1.0, -2.0, 0.5);
  OccupancyMap m(origin, "test_frame", 0.1, 5, 5, 5, 0.0f);
  m.SetIndex(2, 2, 2, 1.0f);
  const SignedDistanceField sdf = ExtractSignedDistanceField(m, {});
  const auto world = [&](double gx, double gy, double gz) {
    return std::vector<double>{origin(0, 0) * gx + origin(0, 1) * gy + origin(0, 2) * gz + origin(0, 3),
                               origin(1, 0) * gx + origin(1, 1) * gy + origin(1, 2) * gz + origin(1, 3),
                               origin(2, 0) * gx + origin(2, 1) * gy + origin(2, 2) * gz + origin(2, 3)};
  };
  std::vector<double> q;
  for (const std::vector<double>& p : {world(0.28, 0.26, 0.25),    // inside the voxel, off its centre
                                       world(3.0, 0.25, 0.25),     // outside the grid
                                       world(0.25, 0.25, 0.25),    // the voxel's centre: the gradient is zero
                                       world(0.35, 0.25, 0.25)})   // the centre of a face neighbour: already clear
    q.insert(q.end(), p.begin(), p.end());
  const DistanceEstimates before = EstimateLocationDistances(sdf, q);
  CHECK(before.has_value[0] == 1 && before.distance[0] <= 0.0);

  // The whole filled cell has the centre's (zero) coarse gradient, so every start in it is FLAT_GRADIENT ...
  const ProjectedPositions flat = ProjectLocationsOutOfCollision(sdf, q);
  CHECK(flat.position.size() == 12 && flat.has_value.size() == 4 && flat.status.size() == 4 && flat.iterations.size() == 4);
  CHECK(flat.status[0] == VGT_HIP_PROJECT_FLAT_GRADIENT && flat.has_value[0] == 0 && std::isnan(flat.position[0]));
  CHECK(flat.status[1] == VGT_HIP_PROJECT_OUTSIDE && flat.has_value[1] == 1 && flat.iterations[1] == 0);
  CHECK(std::memcmp(&flat.position[3], &q[3], 3 * sizeof(double)) == 0);
  CHECK(flat.status[2] == VGT_HIP_PROJECT_FLAT_GRADIENT && flat.has_value[2] == 0);
  CHECK(std::isnan(flat.position[6]) && std::isnan(flat.position[7]) && std::isnan(flat.position[8]));
  CHECK(flat.status[3] == VGT_HIP_PROJECT_OK && flat.has_value[3] == 1 && flat.iterations[3] == 0);
  CHECK(std::memcmp(&flat.position[9], &q[9], 3 * sizeof(double)) == 0);

  // ... and a start in a free cell beside it that is closer to the voxel than a clearance walks out to that clearance
  const std::vector<double> near = world(0.31, 0.26, 0.25);
  const double clearance = 0.08;
  const DistanceEstimates near_before = EstimateLocationDistances(sdf, near);
  CHECK(near_before.has_value[0] == 1 && near_before.distance[0] <= clearance);
  const ProjectedPositions out = ProjectLocationsOutOfCollision(sdf, near, clearance);
  CHECK(out.status[0] == VGT_HIP_PROJECT_OK && out.has_value[0] == 1 && out.iterations[0] >= 1);
  const DistanceEstimates after = EstimateLocationDistances(sdf, out.position);
  CHECK(after.has_value[0] == 1 && after.distance[0] > clearance);
  // it moved along the grid's +x, which is (0.8, 0.6, 0) in the world
  const double dx = out.position[0] - near[0], dy = out.position[1] - near[1], dz = out.position[2] - near[2];
  CHECK(dx > 0.0 && dy > 0.0 && std::abs(dz) < 1e-12 && std::abs(dx * 0.6 - dy * 0.8) < 1e-9);
  CHECK(std::sqrt(dx * dx + dy * dy + dz * dz) <= out.iterations[0] * 0.1 * 0.1 * (1 + 1e-12));
  // a limit of one step is reported, not thrown
  const ProjectedPositions limited = ProjectLocationsOutOfCollision(sdf, near, clearance, 0.1, 1);
  CHECK(limited.status[0] == VGT_HIP_PROJECT_ITERATION_LIMIT && limited.has_value[0] == 0 && limited.iterations[0] == 1);
  CHECK(ThrowsInvalidArgument([&] { ProjectLocationsOutOfCollision(sdf, near, clearance, 0.0); }));
  CHECK(ThrowsInvalidArgument([&] { ProjectLocationsOutOfCollision(sdf, near, clearance, 0.1, -1); }));
  return g_failures;
}

int main(int argc, char** argv)
{
  const bool no_device = argc > 1 && std::strcmp(argv[1], "--no-device") == 0;
  const int failures = no_device ? RunNoDevice() : (RunNoDevice(), RunDevice());
  if (failures == 0) std::printf("PASSED\n");
  return failures == 0 ? 0 : 1;
}
