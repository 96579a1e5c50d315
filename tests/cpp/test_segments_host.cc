// CastSegments of the C++ host layer (include/vgt_hip/segment_queries.hpp) on maps under an origin transform that
// rotates and translates: the answers written out by hand, and equality with the C ABI called directly.
//   test_segments_host              needs a HIP device
//   test_segments_host --no-device  only the argument errors that are raised before a device is touched
#include <vgt_hip.h>
#include <vgt_hip/hip_pointcloud_voxelizer.hpp>
#include <vgt_hip/segment_queries.hpp>

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
  const double nan = std::numeric_limits<double>::quiet_NaN();
  OccupancyMap map(Isometry3::Identity(), "f", 1.0, 4, 4, 4, 0.0f);
  SignedDistanceField sdf;
  sdf.grid = DenseGrid(Isometry3::Identity(), "f", 1.0, 4, 4, 4, 1.0f);
  const std::vector<double> one = {0.5, 0.5, 0.5, 3.5, 3.5, 3.5};
  CHECK(ThrowsInvalidArgument([&] { CastSegments(map, {0.1, 0.2, 0.3, 0.4, 0.5}); }));
  CHECK(ThrowsInvalidArgument([&] { CastSegments(sdf, {0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7}, 0.0); }));
  CHECK(ThrowsInvalidArgument([&] { CastSegments(OccupancyMap(), one); }));
  CHECK(ThrowsInvalidArgument([&] { CastSegments(SignedDistanceField(), one, 0.0); }));
  CHECK(ThrowsInvalidArgument([&] { CastSegments(sdf, one, nan); }));
  // an empty batch needs no device
  const SegmentCasts none = CastSegments(sdf, {}, 0.0, true);
  CHECK(none.status.empty() && none.hit_index.empty() && none.hit_fraction.empty() && none.cells_examined.empty() &&
        none.min_value.empty() && none.min_index.empty());
  CHECK(CastSegments(map, {}).status.empty());
  // the C ABI rejects these before any HIP call, and leaves its outputs alone (the field stands in for a context:
  // a non-null context pointer is not dereferenced before the other checks)
  const float* field = map.GetImmutableRawData().data();
  vgt_hip_ctx* stand_in = reinterpret_cast<vgt_hip_ctx*>(const_cast<float*>(field));
  uint8_t status = 9;
  int32_t hit_index = 9, examined = 9, min_index = 9;
  double fraction = 7.0;
  float min_value = 7.0f;
  const auto call = [&](vgt_hip_ctx* ctx, int64_t nx, double resolution, int32_t mode, double threshold, uint32_t flags,
                        uint8_t* status_out, float* min_value_out) {
    return vgt_hip_cast_segments(ctx, field, nx, 4, 4, resolution, mode, 1, threshold, flags, nullptr, one.data(), 1,
                                 status_out, &hit_index, &fraction, &examined, min_value_out,
                                 mode == VGT_HIP_SEGMENT_SDF_BELOW ? &min_index : nullptr);
  };
  CHECK(call(nullptr, 4, 1.0, 0, 0.0, 0u, &status, nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "null") != nullptr);
  CHECK(call(stand_in, 4, 1.0, 0, 0.0, 0u, nullptr, nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "null") != nullptr);
  CHECK(call(stand_in, -4, 1.0, 0, 0.0, 0u, &status, nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "negative") != nullptr);
  CHECK(call(stand_in, int64_t{1} << 31, 1.0, 0, 0.0, 0u, &status, nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "2^31") != nullptr);
  CHECK(call(stand_in, 4, 0.0, 0, 0.0, 0u, &status, nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "resolution") != nullptr);
  CHECK(call(stand_in, 4, 1.0, 2, 0.0, 0u, &status, nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "mode") != nullptr);
  CHECK(call(stand_in, 4, 1.0, 0, 0.0, 2u, &status, nullptr) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "flag") != nullptr);
  CHECK(call(stand_in, 4, 1.0, 1, nan, 0u, &status, &min_value) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "threshold") != nullptr);
  CHECK(call(stand_in, 4, 1.0, 0, 0.0, 0u, &status, &min_value) == VGT_HIP_ERR_INVALID_ARGUMENT);
  CHECK(std::strstr(vgt_hip_last_error(), "min_value") != nullptr);
  CHECK(status == 9 && hit_index == 9 && examined == 9 && min_index == 9 && fraction == 7.0 && min_value == 7.0f);
  return g_failures;
}

// a, b given in the grid frame -> 6 doubles in the world frame of `origin`
static void Append(std::vector<double>& segments, const Isometry3& origin, const double (&grid)[6])
{
  for (int end = 0; end < 2; end++)
  {
    const double* p = grid + 3 * end;
    for (int row = 0; row < 3; row++)
      segments.push_back(origin(row, 0) * p[0] + origin(row, 1) * p[1] + origin(row, 2) * p[2] + origin(row, 3));
  }
}

template <typename T>
static bool SameBytes(const std::vector<T>& a, const std::vector<T>& b)
{
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

static int RunDevice()
{
  // the grid frame is turned about z and moved
  const double half = 0.5 * 0.6435011087932844;  // cos = 0.8, sin = 0.6
  const Isometry3 origin = Isometry3::FromQuaternion(std::cos(half), 0.0, 0.0, std::sin(half), 1.0, -2.0, 0.5);

  // 1 x 1 x 4 cells of 1, z = 2 filled: the column cast up and down.  (Ends on cell centres in x and y, quarter cells
  // in z: the rounding of the transform cannot move them into another cell.)
  OccupancyMap column(origin, "test_frame", 1.0, 1, 1, 4, 0.0f);
  column.SetIndex(0, 0, 2, 1.0f);
  std::vector<double> up_down;
  Append(up_down, origin, {0.5, 0.5, 0.25, 0.5, 0.5, 3.75});
  Append(up_down, origin, {0.5, 0.5, 3.75, 0.5, 0.5, 0.25});
  const SegmentCasts col = CastSegments(column, up_down);
  CHECK(col.status.size() == 2 && col.min_value.empty() && col.min_index.empty());
  CHECK(col.status[0] == VGT_HIP_SEGMENT_HIT && col.hit_index[0] == 2 && col.cells_examined[0] == 3);
  CHECK(std::abs(col.hit_fraction[0] - 0.5) < 1e-12);
  CHECK(col.status[1] == VGT_HIP_SEGMENT_HIT && col.hit_index[1] == 2 && col.cells_examined[1] == 2);
  CHECK(std::abs(col.hit_fraction[1] - 0.75 / 3.5) < 1e-12);

  // 4^3 cells of 1, empty
  OccupancyMap empty(origin, "test_frame", 1.0, 4, 4, 4, 0.0f);
  std::vector<double> seg;
  Append(seg, origin, {-1.5, 0.5, 0.5, 5.5, 0.5, 0.5});   // through the grid: x = 0..3
  Append(seg, origin, {-3.0, 0.5, 0.5, -1.0, 0.5, 0.5});  // ends before the grid
  Append(seg, origin, {5.5, 0.5, 0.5, 4.5, 0.5, 0.5});    // ends before the grid, from above
  Append(seg, origin, {3.5, 0.5, 0.5, 4.5, 0.5, 0.5});    // leaves through the upper face: one cell
  Append(seg, origin, {1.5, 2.5, 3.5, 1.5, 2.5, 3.5});    // length zero inside: one cell
  Append(seg, origin, {-1.0, 0.5, 0.5, -1.0, 0.5, 0.5});  // length zero outside
  Append(seg, origin, {0.5, 0.5, 0.5, 3.5, 3.4, 3.3});    // a diagonal: 3 + 3 + 3 steps, 10 cells
  seg.insert(seg.end(), {0.0, std::numeric_limits<double>::quiet_NaN(), 0.0, 1.0, 1.0, 1.0});
  seg.insert(seg.end(), {0.0, 0.0, 0.0, std::numeric_limits<double>::infinity(), 1.0, 1.0});
  const SegmentCasts got = CastSegments(empty, seg);
  const uint8_t want_status[9] = {0, 2, 2, 0, 0, 2, 0, 3, 3};
  const int32_t want_examined[9] = {4, 0, 0, 1, 1, 0, 10, 0, 0};
  CHECK(got.status.size() == 9);
  for (size_t i = 0; i < 9 && i < got.status.size(); i++)
  {
    CHECK(got.status[i] == want_status[i]);
    CHECK(got.cells_examined[i] == want_examined[i]);
    CHECK(got.hit_index[i] == -1 && std::isnan(got.hit_fraction[i]));
  }
  // the order of examination: fill the k-th cell of the x line and the cast stops there after k + 1 cells
  for (int k = 0; k < 4; k++)
  {
    OccupancyMap line(origin, "test_frame", 1.0, 4, 4, 4, 0.0f);
    line.SetIndex(k, 0, 0, 0.5f);
    const std::vector<double> through(seg.begin(), seg.begin() + 6);
    const SegmentCasts hit = CastSegments(line, through);
    CHECK(hit.status[0] == VGT_HIP_SEGMENT_HIT && hit.hit_index[0] == k * 16 && hit.cells_examined[0] == k + 1);
    CHECK(std::abs(hit.hit_fraction[0] - (1.5 + k) / 7.0) < 1e-12);
    const SegmentCasts unknown_free = CastSegments(line, through, false);
    CHECK(unknown_free.status[0] == VGT_HIP_SEGMENT_CLEAR && unknown_free.cells_examined[0] == 4);
  }

  // the SDF of the 4^3 map with (2, 0, 0) filled: clearance of the x line, and equality with the C ABI called directly
  OccupancyMap one(origin, "test_frame", 1.0, 4, 4, 4, 0.0f);
  one.SetIndex(2, 0, 0, 1.0f);
  const SignedDistanceField sdf = ExtractSignedDistanceField(one, {});
  for (const bool walk_through : {false, true})
  {
    const SegmentCasts cast = CastSegments(sdf, seg, 0.0, walk_through);
    CHECK(cast.min_value.size() == 9 && cast.min_index.size() == 9);
    CHECK(cast.status[0] == VGT_HIP_SEGMENT_HIT && cast.hit_index[0] == 32);
    CHECK(cast.cells_examined[0] == (walk_through ? 4 : 3));
    CHECK(cast.min_index[0] == 32 && cast.min_value[0] < 0.0f);
    CHECK(cast.status[7] == VGT_HIP_SEGMENT_INVALID && cast.min_index[7] == -1 && std::isnan(cast.min_value[7]));
    SegmentCasts direct;
    direct.status.resize(9);
    direct.hit_index.resize(9);
    direct.cells_examined.resize(9);
    direct.hit_fraction.resize(9);
    direct.min_value.resize(9);
    direct.min_index.resize(9);
    vgt_hip_ctx* ctx = nullptr;
    CHECK(vgt_hip_create(0, -1, &ctx) == VGT_HIP_OK);
    const DenseGrid& g = sdf.grid;
    CHECK(vgt_hip_cast_segments(ctx, g.GetImmutableRawData().data(), 4, 4, 4, 1.0, VGT_HIP_SEGMENT_SDF_BELOW, 1, 0.0,
                                walk_through ? VGT_HIP_SEGMENT_WALK_THROUGH : 0u, g.InverseOriginTransform().m.data(),
                                seg.data(), 9, direct.status.data(), direct.hit_index.data(), direct.hit_fraction.data(),
                                direct.cells_examined.data(), direct.min_value.data(), direct.min_index.data()) == VGT_HIP_OK);
    vgt_hip_destroy(ctx);
    CHECK(SameBytes(cast.status, direct.status) && SameBytes(cast.hit_index, direct.hit_index));
    CHECK(SameBytes(cast.cells_examined, direct.cells_examined) && SameBytes(cast.hit_fraction, direct.hit_fraction));
    CHECK(SameBytes(cast.min_value, direct.min_value) && SameBytes(cast.min_index, direct.min_index));
  }
  // a clearance no cell of the line has: clear, and the least distance is reported
  const std::vector<double> far_line = [&] {
    std::vector<double> s;
    Append(s, origin, {0.5, 3.5, 3.5, 3.5, 3.5, 3.5});
    return s;
  }();
  const SegmentCasts clear = CastSegments(sdf, far_line, 1.0, true);
  CHECK(clear.status[0] == VGT_HIP_SEGMENT_CLEAR && clear.cells_examined[0] == 4 && clear.min_value[0] > 1.0f);
  CHECK(ThrowsInvalidArgument([&] { CastSegments(sdf, far_line, std::numeric_limits<double>::quiet_NaN()); }));
  return g_failures;
}

int main(int argc, char** argv)
{
  const bool no_device = argc > 1 && std::strcmp(argv[1], "--no-device") == 0;
  const int failures = no_device ? RunNoDevice() : (RunNoDevice(), RunDevice());
  if (failures == 0) std::printf("PASSED\n");
  return failures == 0 ? 0 : 1;
}
