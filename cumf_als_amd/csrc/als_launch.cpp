// als_launch.cpp -- carries out a route: the per-NB entry points of the kernel files (als_internal.h) for the run-time
// feature-block count, the standalone batched solvers, and the optional HIP-event timing of the launch sequences.
// Host only: every kernel is launched by the kernel files' own launchers.
#include <atomic>
#include <mutex>
#include <vector>

#include "als_internal.h"

namespace cumf {

// ---- Optional per-kernel HIP-event timing (bench.py's roofline leg): events are recorded on the SAME stream the
// kernels are launched on.  Every timed launch sequence takes the next event triple of a pool, so that the launches of
// a half-iteration made of several -- X_BATCH / THETA_BATCH plans, the pipeline pieces of the multi-GPU gather scheme --
// can be summed afterwards (kernel_ms_since_reset).
namespace {
struct TimedLaunch {
  hipEvent_t ev[3];  // item phase ev[0] -> ev[1], chunked rows' solver ev[1] -> ev[2]
  bool item, reduce;  // which of the two phases ran
};
constexpr size_t kTimedPool = 1024;
bool g_timing = false;
std::vector<TimedLaunch> g_timed;  // pool of event triples, created on first use
size_t g_timed_used = 0;           // launches since the last reset
TimedLaunch* g_newest = nullptr;   // the newest timed launch (last_kernel_ms), kept across resets
std::mutex g_timed_mutex;

// the pool entry of a new launch sequence; nullptr when timing is off
TimedLaunch* timing_begin() {
  if (!g_timing) return nullptr;
  std::lock_guard<std::mutex> lock(g_timed_mutex);
  if (g_timed_used == kTimedPool) g_timed_used = 0;  // nobody read for 1024 launches: start over
  g_newest = &g_timed[g_timed_used++];
  return g_newest;
}

// the Gram(+solve) kernel the last half-iteration dispatched (bench.py reads its name for roofline.kernel)
std::atomic<const void*> g_last_item_kernel{nullptr};
}  // namespace

void set_kernel_timing(bool on) {
  std::lock_guard<std::mutex> lock(g_timed_mutex);
  g_timing = on;
  if (on && g_timed.empty()) {
    g_timed.resize(kTimedPool);
    for (auto& t : g_timed) {
      for (auto& e : t.ev) (void)hipEventCreate(&e);
      t.item = t.reduce = false;
    }
  }
}
hipError_t last_kernel_ms(float* item_ms, float* reduce_ms) {
  *item_ms = 0.f;
  *reduce_ms = 0.f;
  const TimedLaunch* t = g_newest;
  if (!t) return hipSuccess;
  hipError_t e = hipEventSynchronize(t->ev[2]);
  if (e != hipSuccess) return e;
  if (t->item) (void)hipEventElapsedTime(item_ms, t->ev[0], t->ev[1]);
  if (t->reduce) (void)hipEventElapsedTime(reduce_ms, t->ev[1], t->ev[2]);
  return hipSuccess;
}
hipError_t kernel_ms_since_reset(float* item_ms, float* reduce_ms, int* launches) {
  std::lock_guard<std::mutex> lock(g_timed_mutex);
  *item_ms = 0.f;
  *reduce_ms = 0.f;
  *launches = (int)g_timed_used;
  for (size_t i = 0; i < g_timed_used; ++i) {
    TimedLaunch& t = g_timed[i];
    hipError_t e = hipEventSynchronize(t.ev[2]);
    if (e != hipSuccess) return e;
    float ms = 0.f;
    if (t.item && hipEventElapsedTime(&ms, t.ev[0], t.ev[1]) == hipSuccess) *item_ms += ms;
    if (t.reduce && hipEventElapsedTime(&ms, t.ev[1], t.ev[2]) == hipSuccess) *reduce_ms += ms;
  }
  g_timed_used = 0;
  return hipSuccess;
}

void note_item_kernel(const void* host_function) { g_last_item_kernel.store(host_function, std::memory_order_relaxed); }
const void* last_item_kernel() { return g_last_item_kernel.load(std::memory_order_relaxed); }

// ---- Half-iteration
// the wave kernels of one launch, by NB (als_wave.hip)
static hipError_t wave_items(const KernelArgs& a, int mode, const Route& r, bool whole, long n_items, hipStream_t stream) {
  return with_nb<2, kMaxWaveNB>(nb_for_f(a.f), [&](auto nb) { return wave_item_launch<nb>(a, mode, r, whole, n_items, stream); });
}

// One-wave path: the items of the plan (Route::n_short, Route::chunk_first), then launch_half_iteration's reduce phase
static hipError_t one_wave_items(const KernelArgs& a, int mode, const Route& r, const PlanLists& L, hipStream_t stream) {
  KernelArgs aw = a;
  long n_items = L.n_items;
  if (r.chunk_first) {
    aw.item_row = L.w_row, aw.item_begin = L.w_begin, aw.item_len = L.w_len;
    aw.item_slot = nullptr, aw.item_rowlen = L.w_rowlen;
    n_items = L.n_witems;
  }
  if (r.n_short > 0) {  // the last items; first: the tail of the long items then fills in behind it
    n_items -= r.n_short;
    KernelArgs as = aw;
    as.item_row += n_items, as.item_begin += n_items, as.item_len += n_items, as.item_rowlen += n_items;
    hipError_t e = launch_short_cg(as, r.n_short, stream);
    if (e != hipSuccess) return e;
  }
  if (r.chunk_first) {
    KernelArgs ac = a;
    ac.item_row = L.c_row, ac.item_begin = L.c_begin, ac.item_len = L.c_len;
    ac.item_slot = L.c_slot, ac.item_rowlen = L.c_rowlen;
    hipError_t e = wave_items(ac, mode, r, false, L.n_citems, stream);
    if (e != hipSuccess) return e;
  }
  return wave_items(aw, mode, r, r.chunk_first || L.n_mrows == 0, n_items, stream);
}

hipError_t launch_half_iteration(const KernelArgs& a, int mode, const Route& r, const PlanLists& L, hipStream_t stream) {
  const int nb = nb_for_f(a.f);
  // item phase (event 0 -> 1), then the chunked rows' solver (1 -> 2); the two-wave path interleaves them (item phase only)
  TimedLaunch* t = timing_begin();
  if (t) {
    t->item = r.path == kPathTwoWave || L.n_items > 0;
    t->reduce = r.path != kPathTwoWave && L.n_mrows > 0;
    (void)hipEventRecord(t->ev[0], stream);
  }
  hipError_t e = hipErrorInvalidValue;
  switch (r.path) {
    case kPathTwoWave:
      e = with_nb<kMaxWaveNB + 1, kMaxNB>(nb, [&](auto n) { return slice_batched<n>(a, mode, r, L, stream); });
      break;
    case kPathOneWave: e = one_wave_items(a, mode, r, L, stream); break;
    case kPathWorkgroup:
      e = with_nb<1, kMaxNB>(nb, [&](auto n) { return slice_half_iteration<n>(a, mode, L.n_items, 0, stream); });
      break;
    default: break;
  }
  if (t) (void)hipEventRecord(t->ev[1], stream);
  if (e == hipSuccess && r.path != kPathTwoWave && L.n_mrows > 0) {
    e = with_nb<1, kMaxNB>(nb, [&](auto n) {
      return r.path == kPathOneWave ? slice_reduce_only<n>(a, mode, r, L.n_mrows, stream)
                                    : slice_half_iteration<n>(a, mode, 0, L.n_mrows, stream);
    });
  }
  if (t) (void)hipEventRecord(t->ev[2], stream);
  return e;
}

hipError_t launch_solve_batched(const float* A, const float* b, float* x, long batch, int f, int mode, int cg_iters,
                                hipStream_t stream) {
  if (batch <= 0) return hipSuccess;
  if (mode == kModeLUExact) return slice_solve<0>(A, b, x, batch, f, mode, 0, stream);
  if (f > 128 && (mode == kModeCG || mode == kModeCGHalf))  // system too large for the LDS: A streamed from global memory
    return launch_cg_global(A, b, x, batch, f, cg_iters, mode == kModeCGHalf, stream);
  // LDS-resident CG (f <= 128) or register-resident LU (f <= 200)
  return with_nb<1, kMaxNB>(nb_for_f(f), [&](auto n) { return slice_solve<n>(A, b, x, batch, f, mode, cg_iters, stream); });
}

}  // namespace cumf
