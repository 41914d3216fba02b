// als_scratch.cpp -- the process-wide scratch pool of the entry points and the per-device range flag of gram mode "fast"
// (cumf_release_scratch and cumf_gram_fast_status of include/cumf_als_capi.h).  The mutex, the maps and the condition variable
// are private to this file.
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstdio>
#include <map>
#include <mutex>
#include <tuple>

#include "als_internal.h"
#include "cumf_als_capi.h"

using namespace cumf;

namespace {

// Scratch that outlives a call: the dense-slot tile buffer of the batched path (up to 48 GiB) and the pre-split
// copy of the gather table (gram mode "fast").  Process-wide, grow-only, one buffer per (device, stream, kind):
// calls on one stream are ordered, so the X_BATCH / THETA_BATCH plans of doALS and the pipeline pieces of
// DistALS share ONE buffer instead of keeping one each.  cumf_release_scratch frees them.
struct Scratch {
  void* ptr = nullptr;
  size_t cap = 0;
};
std::mutex g_scratch_mutex;
std::map<std::tuple<int, hipStream_t, int>, Scratch> g_scratch;
std::map<int, int*> g_fast_flag;  // per device (range report of gram mode "fast")
// Host threads that are inside a launch sequence using pooled pointers, per device (a second host thread
// between its Gram launch and its reduce / LU launch must not have its tile buffer freed by another thread's
// cumf_release_scratch).  An entry point that takes pooled scratch holds a ScratchLease until its last launch is
// enqueued; cumf_release_scratch waits until no lease of its device is held, then synchronises the device (the
// enqueued kernels finish) and frees that device's entries only.
std::map<int, int> g_scratch_users;
std::condition_variable g_scratch_cv;

}  // namespace

cumf::ScratchLease::ScratchLease() {
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(g_scratch_mutex);
  ++g_scratch_users[dev];
}
cumf::ScratchLease::~ScratchLease() {
  {
    std::lock_guard<std::mutex> lock(g_scratch_mutex);
    --g_scratch_users[dev];
  }
  g_scratch_cv.notify_all();
}

int cumf::scratch_get(hipStream_t stream, int kind, size_t bytes, void** out) {
  int dev = 0;
  CUMF_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(g_scratch_mutex);
  Scratch& sc = g_scratch[std::make_tuple(dev, stream, kind)];
  if (sc.cap < bytes) {
    if (sc.ptr) {
      CUMF_HIP_CHECK(hipStreamSynchronize(stream));  // kernels of earlier calls may still read it
      CUMF_HIP_CHECK(hipFree(sc.ptr));
      sc.ptr = nullptr;
      sc.cap = 0;
    }
    CUMF_HIP_CHECK(hipMalloc(&sc.ptr, bytes));
    sc.cap = bytes;
  }
  *out = sc.ptr;
  return 0;
}

size_t cumf::scratch_capacity(hipStream_t stream, int kind) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(g_scratch_mutex);
  auto have = g_scratch.find(std::make_tuple(dev, stream, kind));
  return have != g_scratch.end() ? have->second.cap : 0;
}

int cumf::fast_flag_get(int** out) {
  int dev = 0;
  CUMF_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(g_scratch_mutex);
  int*& flag = g_fast_flag[dev];
  if (!flag) {
    CUMF_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&flag), sizeof(int)));
    CUMF_HIP_CHECK(hipMemset(flag, 0, sizeof(int)));
  }
  *out = flag;
  return 0;
}

// Range report of gram mode "fast" since the last call (waits for the device): bit 0 = a factor beyond
// the f16 range of the pre-split table, bit 1 = a rating beyond it (the affected rows are not finite).
extern "C" int cumf_gram_fast_status(int* flags) {
  if (!flags) return (int)hipErrorInvalidValue;
  *flags = 0;
  int dev = 0;
  CUMF_HIP_CHECK(hipGetDevice(&dev));
  int* flag = nullptr;
  {
    std::lock_guard<std::mutex> lock(g_scratch_mutex);
    auto it = g_fast_flag.find(dev);
    if (it != g_fast_flag.end()) flag = it->second;
  }
  if (!flag) return 0;
  CUMF_HIP_CHECK(hipDeviceSynchronize());  // every stream: no kernel is OR-ing into the flag any more
  CUMF_HIP_CHECK(hipMemcpy(flags, flag, sizeof(int), hipMemcpyDeviceToHost));
  CUMF_HIP_CHECK(hipMemset(flag, 0, sizeof(int)));
  return 0;
}

// Frees the pooled scratch of the CURRENT device (tile buffers, pre-split tables, range flag; all streams); doALS
// calls it on exit.  Waits for host threads that are inside a launch sequence on this device (ScratchLease) and for
// the device itself; other devices' entries are left alone.
extern "C" int cumf_release_scratch(void) {
  int dev = 0;
  CUMF_HIP_CHECK(hipGetDevice(&dev));
  std::unique_lock<std::mutex> lock(g_scratch_mutex);
  g_scratch_cv.wait(lock, [&] { return g_scratch_users[dev] == 0; });
  CUMF_HIP_CHECK(hipDeviceSynchronize());
  for (auto it = g_scratch.begin(); it != g_scratch.end();) {
    if (std::get<0>(it->first) == dev) {
      if (it->second.ptr) (void)hipFree(it->second.ptr);
      it = g_scratch.erase(it);
    } else {
      ++it;
    }
  }
  auto ff = g_fast_flag.find(dev);
  if (ff != g_fast_flag.end()) {
    if (ff->second) (void)hipFree(ff->second);
    g_fast_flag.erase(ff);
  }
  return 0;
}
