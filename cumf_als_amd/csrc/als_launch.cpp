// als_launch.cpp -- carries out a route (workgroup, one-wave or two-wave path): which per-NB entry points of the kernel files
// (als_internal.h) run on which item lists, for the run-time feature-block count; the standalone batched solvers; and the
// optional HIP-event timing of the launch sequences; the tile-batch probe (cumf_last_tile_batches).
// Host only: every kernel is launched by the kernel files' own launchers.
#include <atomic>
#include <mutex>
#include <vector>

#include "als_internal.h"
#include "cumf_als_capi.h"

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

// batches of the pooled tile buffer the newest launch_half_iteration carried out (0: it did not go through the buffer) and
// the rows of one batch (PlanLists::part2_rows): cumf_last_tile_batches
std::atomic<long> g_tile_batches{0}, g_tile_batch_rows{0};
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
// the wave kernels of one launch, by NB (als_wave.hip): one wave per item up to kMaxWaveNB, two above
static hipError_t wave_items(const KernelArgs& a, int mode, const Route& r, bool whole, long n_items, hipStream_t stream) {
  return with_nb<2, kMaxNB>(nb_for_f(a.f), [&](auto nb) { return wave_item_launch<nb>(a, mode, r, whole, n_items, stream); });
}
// the solver of the chunked rows on its own (als_kernels.hip)
static hipError_t reduce_rows(const KernelArgs& a, int mode, const Route& r, long n_mrows, hipStream_t stream) {
  return with_nb<1, kMaxNB>(nb_for_f(a.f), [&](auto nb) { return slice_reduce_only<nb>(a, mode, r, n_mrows, stream); });
}

// The item lists of a launch: the plan's whole rows from row w0 of the w list on (no slots: nothing is dumped by slot) ...
static KernelArgs whole_row_items(KernelArgs a, const PlanLists& L, long w0 = 0) {
  a.item_row = L.w_row + w0, a.item_begin = L.w_begin + w0, a.item_len = L.w_len + w0;
  a.item_slot = nullptr, a.item_rowlen = L.w_rowlen + w0;
  return a;
}
// ... or its chunk items, each with its slot of the plan's partial tiles
static KernelArgs chunk_items(KernelArgs a, const PlanLists& L) {
  a.item_row = L.c_row, a.item_begin = L.c_begin, a.item_len = L.c_len;
  a.item_slot = L.c_slot, a.item_rowlen = L.c_rowlen;
  return a;
}

// One-wave path: the items of the plan (Route::n_short, Route::chunk_first), then launch_half_iteration's reduce phase
static hipError_t one_wave_items(const KernelArgs& a, int mode, const Route& r, const PlanLists& L, hipStream_t stream) {
  const KernelArgs aw = r.chunk_first ? whole_row_items(a, L) : a;
  long n_items = r.chunk_first ? L.n_witems : L.n_items;
  if (r.n_short > 0) {  // the last items; first: the tail of the long items then fills in behind it
    n_items -= r.n_short;
    KernelArgs as = aw;
    as.item_row += n_items, as.item_begin += n_items, as.item_len += n_items, as.item_rowlen += n_items;
    hipError_t e = launch_short_cg(as, r.n_short, stream);
    if (e != hipSuccess) return e;
  }
  // Route::n_dual: the whole rows of 1 .. kDualMaxRow ratings, the last of the list but for the n_dual_behind rows without
  // ratings, on their dual form -- first, like the short rows of the CG; the rows behind them in a wave launch of their own
  // (the plan lists them there in the full list too: a combined launch of chunk items and whole rows hands them over alike)
  const bool whole = r.chunk_first || L.n_mrows == 0;
  const bool dual = r.n_dual > 0 && mode == kModeLU && !a.dense_slots && r.n_dual + r.n_dual_behind <= n_items;
  long n_behind = 0;
  if (dual) {
    n_behind = r.n_dual_behind;
    n_items -= r.n_dual + n_behind;
    KernelArgs ad = aw;
    ad.item_row += n_items, ad.item_begin += n_items, ad.item_len += n_items, ad.item_rowlen += n_items;
    hipError_t e = launch_dual_rows(ad, r.n_dual, stream);
    if (e != hipSuccess) return e;
  }
  if (r.chunk_first) {
    hipError_t e = wave_items(chunk_items(a, L), mode, r, false, L.n_citems, stream);
    if (e != hipSuccess) return e;
  }
  if (n_behind > 0) {
    const long at = n_items + r.n_dual;
    KernelArgs ab = aw;
    ab.item_row += at, ab.item_begin += at, ab.item_len += at, ab.item_rowlen += at;
    if (ab.item_slot) ab.item_slot += at;
    hipError_t e = wave_items(ab, mode, r, whole, n_behind, stream);
    if (e != hipSuccess) return e;
  }
  return wave_items(aw, mode, r, whole, n_items, stream);
}

// Two-wave path (f >= 112): the Gram of every row is dumped as accumulator tiles (two waves per item,
// als_wave_multi_kernel) and a solver kernel (single-wave LU up to NB = 10, the 4-wave lu_solve_mfma
// above that, wave-level CG on the tiles) picks them up -- the reference's own data flow ("Gram batch
// in device memory, separate solver", als.cu:782-831), with tiles instead of full f x f matrices and
// in batches of the pooled tile buffer (als_plan.cpp: up to 48 GiB, usually ONE batch).
static hipError_t two_wave_items(const KernelArgs& a0, int mode, const Route& r, const PlanLists& L, hipStream_t stream) {
  hipError_t e = hipSuccess;
  // 1. chunked rows: their items write the plan's slots, the reduce kernel sums and solves
  if (L.n_citems > 0) {
    e = wave_items(chunk_items(a0, L), kModeLU, r, false, L.n_citems, stream);  // every item has a slot: nothing is solved in place
    if (e != hipSuccess) return e;
    e = reduce_rows(a0, mode, r, L.n_mrows, stream);
    if (e != hipSuccess) return e;
  }
  // 2. whole rows: solved by the two waves that formed the Gram, in one launch, or through the tile buffer
  if (r.whole == kSolveInKernel) {
    if (L.n_witems <= 0) return hipSuccess;
    KernelArgs a = whole_row_items(a0, L);
    a.dense_slots = 0;
    return wave_items(a, mode, r, false, L.n_witems, stream);
  }
  // large LU / materialise (cumf_get_hermitian): in batches of part2_rows dense slots
  for (long w0 = 0; w0 < L.n_witems; w0 += L.part2_rows) {
    g_tile_batches.fetch_add(1, std::memory_order_relaxed);
    const long cnt = L.n_witems - w0 < L.part2_rows ? L.n_witems - w0 : L.part2_rows;
    KernelArgs a = whole_row_items(a0, L, w0);
    a.dense_slots = 1;
    a.part = L.part2;
    a.mrow_row = L.w_row + w0;
    a.mrow_rowlen = L.w_rowlen + w0;
    e = wave_items(a, kModeLU, r, false, cnt, stream);
    if (e != hipSuccess) return e;
    e = reduce_rows(a, mode, r, cnt, stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_half_iteration(const KernelArgs& a, int mode, const Route& r, const PlanLists& L, hipStream_t stream) {
  const int nb = nb_for_f(a.f);
  g_tile_batches.store(0, std::memory_order_relaxed);
  g_tile_batch_rows.store(L.part2_rows, std::memory_order_relaxed);
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
      e = nb > kMaxWaveNB ? two_wave_items(a, mode, r, L, stream) : hipErrorInvalidValue;
      break;
    case kPathOneWave: e = one_wave_items(a, mode, r, L, stream); break;
    case kPathWorkgroup:
      e = with_nb<1, kMaxNB>(nb, [&](auto n) { return slice_half_iteration<n>(a, mode, L.n_items, 0, stream); });
      break;
    default: break;
  }
  if (t) (void)hipEventRecord(t->ev[1], stream);
  if (e == hipSuccess && r.path != kPathTwoWave && L.n_mrows > 0) {
    e = r.path == kPathOneWave
            ? reduce_rows(a, mode, r, L.n_mrows, stream)
            : with_nb<1, kMaxNB>(nb, [&](auto n) { return slice_half_iteration<n>(a, mode, 0, L.n_mrows, stream); });
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

// Plain host state, no HIP call: how the newest launch_half_iteration of this process used the pooled tile buffer.
extern "C" int cumf_last_tile_batches(long info[2]) {
  if (!info) return (int)hipErrorInvalidValue;
  info[0] = cumf::g_tile_batches.load(std::memory_order_relaxed);
  info[1] = cumf::g_tile_batch_rows.load(std::memory_order_relaxed);
  return 0;
}
