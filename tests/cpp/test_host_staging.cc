// csrc/host_staging.hpp against the fake runtime of hip_fake/: the order of a successful call, the carving, absent and
// empty arrays, and every failure path (allocation, each upload, the body, each download, the wait), which no GPU test
// can reach.  Sizes: a byte, 3 bytes, 105 floats (a 3 x 5 x 7 grid) and 5 x 3 doubles -- none a multiple of 256, so
// every array after the first starts at a carved boundary.  Stand-alone: prints PASSED or exits non-zero.
#include "../../voxelized_geometry_tools_amd/csrc/host_staging.hpp"

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace
{
using hip_fake::Kind;

int g_failures = 0;
#define CHECK(cond)                                                       \
  do                                                                      \
  {                                                                       \
    if (!(cond))                                                          \
    {                                                                     \
      std::printf("%s:%d: [%s] %s\n", __FILE__, __LINE__, g_case, #cond); \
      g_failures++;                                                       \
    }                                                                     \
  } while (0)
const char* g_case = "";

struct Context
{
  std::mutex mutex;
  hipStream_t stream = reinterpret_cast<hipStream_t>(0x51);
};

const char* g_failed_what = nullptr;
int FailCode(const char* what, hipError_t err)
{
  g_failed_what = what;
  return 1000 + static_cast<int>(err);
}

constexpr uint8_t kSentinel = 0xEE;
constexpr size_t kFloats = 3 * 5 * 7, kDoubles = 5 * 3;

// The caller's side of one call: a byte and an empty array to upload, 3 bytes and 5 x 3 doubles to download, 105 floats
// both ways, an output nobody asked for, and scratch.
struct Call
{
  uint8_t flag[1] = {7};
  uint8_t empty[1] = {9};
  uint8_t three[3] = {kSentinel, kSentinel, kSentinel};
  std::vector<float> grid = std::vector<float>(kFloats);
  std::vector<double> rows = std::vector<double>(kDoubles, -1.0);
  bool body_ran = false;
  size_t log_at_body = 0;

  Call()
  {
    for (size_t i = 0; i < kFloats; i++) grid[i] = static_cast<float>(i);
  }

  // Declares, runs (under the context's mutex, or with the test holding it), lets the staging object go.
  int Run(Context& ctx, bool locked, int body_result)
  {
    vgt::HostStaging staging;
    const auto flag_dev = staging.In(flag, 1);
    const auto three_dev = staging.Out(three, 3);
    const auto absent_dev = staging.Out(static_cast<int32_t*>(nullptr), 5);
    const auto grid_dev = staging.InOut(grid.data(), kFloats);
    const auto empty_dev = staging.In(empty, 0);
    const auto rows_dev = staging.Out(rows.data(), kDoubles);
    const auto scratch_dev = staging.Scratch(33);
    const auto body = [&](hipStream_t s) {
      body_ran = true;
      log_at_body = hip_fake::state().log.size();
      CHECK(s == ctx.stream);
      // the one block, from the log of its allocation
      const hip_fake::Call& block = hip_fake::state().log[0];
      CHECK(block.kind == hip_fake::kMalloc);
      const char* const begin = static_cast<const char*>(block.dst);
      const auto carved = [&](const void* p, size_t bytes) {
        const char* const at = static_cast<const char*>(p);
        return p && reinterpret_cast<uintptr_t>(p) % 256 == 0 && at >= begin && at + bytes <= begin + block.bytes;
      };
      CHECK(carved(flag_dev.dev(), 1));
      CHECK(carved(three_dev.dev(), 3));
      CHECK(carved(grid_dev.dev(), kFloats * sizeof(float)));
      CHECK(carved(empty_dev.dev(), 0));
      CHECK(carved(rows_dev.dev(), kDoubles * sizeof(double)));
      CHECK(carved(scratch_dev.dev(), 33));
      CHECK(absent_dev.dev() == nullptr);
      // what was uploaded is there; write every output to its last element
      CHECK(flag_dev.dev()[0] == 7);
      CHECK(grid_dev.dev()[kFloats - 1] == static_cast<float>(kFloats - 1));
      for (size_t i = 0; i < 3; i++) three_dev.dev()[i] = static_cast<uint8_t>(i + 1);
      for (size_t i = 0; i < kFloats; i++) grid_dev.dev()[i] *= 2.0f;
      for (size_t i = 0; i < kDoubles; i++) rows_dev.dev()[i] = 0.5 * static_cast<double>(i);
      std::memset(scratch_dev.dev(), 0xAB, 33);
      return body_result;
    };
    if (!locked) return staging.Run(ctx, "the call", FailCode, body);
    std::lock_guard<std::mutex> lock(ctx.mutex);  // (RunLocked must not try to take it: that would hang here)
    return staging.RunLocked(ctx.stream, "the call", FailCode, body);
  }

  bool OutputsUntouched() const
  {
    bool same = three[0] == kSentinel && three[1] == kSentinel && three[2] == kSentinel;
    for (size_t i = 0; i < kFloats; i++) same = same && grid[i] == static_cast<float>(i);
    for (size_t i = 0; i < kDoubles; i++) same = same && rows[i] == -1.0;
    return same;
  }
  bool OutputsArrived() const
  {
    bool all = three[0] == 1 && three[1] == 2 && three[2] == 3;
    for (size_t i = 0; i < kFloats; i++) all = all && grid[i] == 2.0f * static_cast<float>(i);
    for (size_t i = 0; i < kDoubles; i++) all = all && rows[i] == 0.5 * static_cast<double>(i);
    return all;
  }
};

std::vector<Kind> KindsLogged()
{
  std::vector<Kind> kinds;
  for (const hip_fake::Call& c : hip_fake::state().log) kinds.push_back(c.kind);
  return kinds;
}

// What holds after every call, whatever failed: one block, freed once and with the mutex free (the staging object
// outlives the lock, Run's own or the test's), nothing live.
void CheckBlockGone()
{
  const hip_fake::State& s = hip_fake::state();
  CHECK(hip_fake::Count(hip_fake::kMalloc) == 1 && hip_fake::Count(hip_fake::kFree) == 1);
  CHECK(s.live_allocations == 0);
  CHECK(s.frees_with_mutex_free == 1 && s.frees_with_mutex_held == 0);
}

void Success(bool locked)
{
  g_case = locked ? "success, RunLocked" : "success, Run";
  Context ctx;
  hip_fake::Reset(&ctx.mutex);
  Call call;
  CHECK(call.Run(ctx, locked, 0) == 0);
  using namespace hip_fake;
  // uploads in declaration order (the empty array is not copied), the body, downloads in declaration order, ONE wait
  const std::vector<Kind> want = {kMalloc, kUpload, kUpload, kDownload, kDownload, kDownload, kSynchronize, kFree};
  CHECK(KindsLogged() == want);
  const std::vector<hip_fake::Call>& log = state().log;
  if (KindsLogged() == want)
  {
    CHECK(call.body_ran && call.log_at_body == 3);
    CHECK(log[1].src == call.flag && log[1].bytes == 1);
    CHECK(log[2].src == call.grid.data() && log[2].bytes == kFloats * sizeof(float));
    CHECK(log[3].dst == call.three && log[3].bytes == 3);
    CHECK(log[4].dst == call.grid.data() && log[4].bytes == kFloats * sizeof(float));
    CHECK(log[5].dst == call.rows.data() && log[5].bytes == kDoubles * sizeof(double));
    for (size_t i = 1; i <= 6; i++) CHECK(log[i].stream == ctx.stream);
    CHECK(log[7].dst == log[0].dst);
  }
  CHECK(call.OutputsArrived());  // (the InOut array among them: what the body wrote)
  CHECK(call.flag[0] == 7 && call.empty[0] == 9);
  CheckBlockGone();
}

void AllocationFails()
{
  g_case = "allocation fails";
  Context ctx;
  hip_fake::Reset(&ctx.mutex);
  hip_fake::FailNth(hip_fake::kMalloc, 1, hipErrorOutOfMemory);
  Call call;
  g_failed_what = nullptr;
  CHECK(call.Run(ctx, false, 0) == 1000 + hipErrorOutOfMemory);
  CHECK(g_failed_what && std::string(g_failed_what) == "the call");
  CHECK(!call.body_ran && call.OutputsUntouched());
  CHECK(KindsLogged() == std::vector<Kind>{hip_fake::kMalloc});  // nothing copied, nothing waited for, nothing to free
  CHECK(hip_fake::state().live_allocations == 0);
}

void UploadFails(int nth, bool locked)
{
  g_case = nth == 1 ? "first upload fails" : "second upload fails";
  Context ctx;
  hip_fake::Reset(&ctx.mutex);
  hip_fake::FailNth(hip_fake::kUpload, nth, hipErrorLaunchFailure);
  hip_fake::FailNth(hip_fake::kSynchronize, 1, hipErrorUnknown);  // (the earlier error is the one reported)
  Call call;
  CHECK(call.Run(ctx, locked, 0) == 1000 + hipErrorLaunchFailure);
  CHECK(!call.body_ran && call.OutputsUntouched());
  CHECK(hip_fake::Count(hip_fake::kUpload) == nth);
  CHECK(hip_fake::Count(hip_fake::kDownload) == 0);
  CHECK(hip_fake::Count(hip_fake::kSynchronize) == 1);
  CheckBlockGone();
}

void BodyFails(bool locked)
{
  g_case = "the body fails";
  Context ctx;
  hip_fake::Reset(&ctx.mutex);
  hip_fake::FailNth(hip_fake::kSynchronize, 1, hipErrorUnknown);  // (the body's code still comes back)
  Call call;
  g_failed_what = nullptr;
  CHECK(call.Run(ctx, locked, 42) == 42);
  CHECK(g_failed_what == nullptr);
  CHECK(call.body_ran && call.OutputsUntouched());  // (the InOut array as the caller gave it)
  CHECK(hip_fake::Count(hip_fake::kDownload) == 0);
  CHECK(hip_fake::Count(hip_fake::kSynchronize) == 1);
  CheckBlockGone();
}

void DownloadFails(int nth, bool locked)
{
  g_case = nth == 1 ? "first download fails" : nth == 2 ? "second download fails" : "third download fails";
  Context ctx;
  hip_fake::Reset(&ctx.mutex);
  hip_fake::FailNth(hip_fake::kDownload, nth, hipErrorLaunchFailure);
  hip_fake::FailNth(hip_fake::kSynchronize, 1, hipErrorUnknown);
  Call call;
  CHECK(call.Run(ctx, locked, 0) == 1000 + hipErrorLaunchFailure);
  CHECK(call.body_ran);
  CHECK(hip_fake::Count(hip_fake::kDownload) == nth);
  CHECK(hip_fake::Count(hip_fake::kSynchronize) == 1);
  CHECK(hip_fake::state().log[hip_fake::state().log.size() - 2].kind == hip_fake::kSynchronize);  // then the free
  CheckBlockGone();
}

void SynchronizeFails(bool locked)
{
  g_case = "the wait fails";
  Context ctx;
  hip_fake::Reset(&ctx.mutex);
  hip_fake::FailNth(hip_fake::kSynchronize, 1, hipErrorUnknown);
  Call call;
  CHECK(call.Run(ctx, locked, 0) == 1000 + hipErrorUnknown);
  CHECK(hip_fake::Count(hip_fake::kSynchronize) == 1);
  CheckBlockGone();
}

// Nothing but outputs nobody asked for: no block at all, and still one unit on the stream.
void NothingToReserve()
{
  g_case = "nothing to reserve";
  Context ctx;
  hip_fake::Reset(&ctx.mutex);
  bool ran = false;
  {
    vgt::HostStaging staging;
    const auto absent = staging.Out(static_cast<double*>(nullptr), kDoubles);
    const auto without = staging.In(static_cast<const float*>(nullptr), kFloats);
    const int rc = staging.Run(ctx, "the call", FailCode, [&](hipStream_t) {
      ran = true;
      CHECK(absent.dev() == nullptr && without.dev() == nullptr);
      return 0;
    });
    CHECK(rc == 0);
  }
  CHECK(ran);
  CHECK(KindsLogged() == std::vector<Kind>{hip_fake::kSynchronize});
}

// More arrays than the fixed slot table holds: refused before anything is allocated.
void TooManyArrays()
{
  g_case = "too many arrays";
  Context ctx;
  hip_fake::Reset(&ctx.mutex);
  bool ran = false;
  {
    vgt::HostStaging staging;
    for (int i = 0; i < 9; i++) (void)staging.Scratch(3);
    const int rc = staging.Run(ctx, "the call", FailCode, [&](hipStream_t) {
      ran = true;
      return 0;
    });
    CHECK(rc == 1000 + hipErrorInvalidValue);
  }
  CHECK(!ran && hip_fake::state().log.empty());
}
}  // namespace

int main()
{
  for (const bool locked : {false, true})
  {
    Success(locked);
    UploadFails(1, locked);
    UploadFails(2, locked);
    BodyFails(locked);
    for (int nth = 1; nth <= 3; nth++) DownloadFails(nth, locked);
    SynchronizeFails(locked);
  }
  AllocationFails();
  NothingToReserve();
  TooManyArrays();
  if (g_failures)
  {
    std::printf("%d checks FAILED\n", g_failures);
    return 1;
  }
  std::printf("PASSED\n");
  return 0;
}
