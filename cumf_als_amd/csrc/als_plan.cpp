// als_plan.cpp -- static work decomposition of one ALS half-iteration + the C ABI of
// the device-pointer entry points (include/cumf_als_capi.h).
//
// The reference launches one CUDA block per row (als.cu:449) inside a per-batch loop
// (als.cu:768-777, 881-890).  On the Netflix X side that is 17 770 rows with up to
// ~230k ratings each over 256 CUs: the tail row alone would run for milliseconds.
// The plan cuts every row into chunks of at most `chunk` ratings ("items"), orders
// the items longest-first and gives each chunk of a split row a slot in a partial
// tile buffer that the reduce kernel sums in slot order (deterministic).
#include <hip/hip_runtime.h>

#include <cxxabi.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <map>
#include <mutex>
#include <numeric>
#include <tuple>
#include <vector>

#include "als_internal.h"
#include "cg.h"
#include "cumf_als_capi.h"

using namespace cumf;


namespace {

int default_chunk(int f, long long nnz) {
  // A chunk of a split row costs a 28 KiB partial-tile write + its share of the reduce (f = 100), so bigger chunks
  // are cheaper as long as every wave slot of the device still gets >= 12 items to balance the tail: 2048 .. 8192
  // ratings depending on the ratings of this side (a 1/8 slab of Netflix on 8 GPUs stays at 2048).  Must be a
  // multiple of kStage.
  (void)f;
  const char* e = getenv("CUMF_ALS_CHUNK");
  int c;
  if (e) {
    c = atoi(e);
  } else {
    int cus = 256;
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const long long slots = (long long)(cus > 0 ? cus : 256) * 4;
    // round 2 (wave-per-item kernels, 2048 wave slots): 4096 -> 8192 saves another 0.35 ms on the Netflix
    // X side (6.84 -> 6.50 ms; 16384: 6.43), still >= 12 items per slot
    const long long want = nnz / (slots * 12);
    c = (int)std::min<long long>(8192, std::max<long long>(2048, want));
  }
  if (c < kStage) c = kStage;
  return (c / kStage) * kStage;
}

}  // namespace

extern "C" int cumf_plan_create(cumf_plan_t** out, const void* rowptr_host, int rowptr_is_64, long rows,
                                long row_begin, long row_end, int f, int chunk) {
  if (!out || !rowptr_host || rows < 0 || row_begin < 0 || row_end > rows || row_begin > row_end) {
    fprintf(stderr, "cumf_plan_create: invalid arguments\n");
    return (int)hipErrorInvalidValue;
  }
  if (f <= 0 || f > kMaxFAny || (f % 2) != 0) {
    fprintf(stderr, "cumf_plan_create: f = %d unsupported (need even f <= %d)\n", f, kMaxFAny);
    return (int)hipErrorInvalidValue;
  }
  auto rp = [&](long i) -> long long {
    return rowptr_is_64 ? static_cast<const long long*>(rowptr_host)[i]
                        : static_cast<long long>(static_cast<const int*>(rowptr_host)[i]);
  };
  // from the ratings of the WHOLE row pointer, not of [row_begin, row_end): the X_BATCH / THETA_BATCH plans
  // of one side then cut their heavy rows alike and a batched run stays bit-identical to the unbatched
  // one (als.cu:768-777; tests/test_gpu_fullsize.py)
  if (chunk <= 0) chunk = default_chunk(f, rp(rows) - rp(0));
  if (f > kMaxF) {
    // above the tile kernels' range (als_generic.hip) a row is never cut: every item is a whole row, there are no partial tiles
    long long longest = 0;
    for (long u = row_begin; u < row_end; ++u) longest = std::max(longest, rp(u + 1) - rp(u));
    chunk = (int)std::min<long long>(0x7fffffe0LL, std::max<long long>(longest, kStage));
    chunk = ((chunk + kStage - 1) / kStage) * kStage;
  }
  chunk = std::max(kStage, (chunk / kStage) * kStage);

  std::vector<int> item_row, item_len, item_slot, item_rowlen;
  std::vector<long long> item_begin;
  std::vector<int> mrow_row, mrow_slot0, mrow_nslots, mrow_rowlen;
  {
    const size_t guess = (size_t)(row_end - row_begin) + (size_t)((rp(row_end) - rp(row_begin)) / chunk) + 16;
    item_row.reserve(guess), item_len.reserve(guess), item_slot.reserve(guess), item_rowlen.reserve(guess);
    item_begin.reserve(guess);
  }
  long n_slots = 0;
  for (long u = row_begin; u < row_end; ++u) {
    const long long s = rp(u), e = rp(u + 1);
    const long long len = e - s;
    if (len < 0 || len > 0x7fffffffLL) {
      fprintf(stderr, "cumf_plan_create: row %ld has invalid length %lld\n", u, len);
      return (int)hipErrorInvalidValue;
    }
    if (len <= chunk) {
      item_row.push_back((int)u);
      item_begin.push_back(s);
      item_len.push_back((int)len);
      item_slot.push_back(-1);
      item_rowlen.push_back((int)len);
    } else {
      const int nchunks = len == 0 ? 1 : (int)((len + chunk - 1) / chunk);
      mrow_row.push_back((int)u);
      mrow_slot0.push_back((int)n_slots);
      mrow_nslots.push_back(nchunks);
      mrow_rowlen.push_back((int)len);
      for (int c = 0; c < nchunks; ++c) {
        const long long b = s + (long long)c * chunk;
        item_row.push_back((int)u);
        item_begin.push_back(b);
        item_len.push_back((int)std::max<long long>(0, std::min<long long>(chunk, e - b)));
        item_slot.push_back((int)(n_slots + c));
        item_rowlen.push_back((int)len);
      }
      n_slots += nchunks;
    }
  }
  // longest-first (stable => deterministic): the hardware dispatches workgroups in
  // index order, so the short items fill the tail.  Item lengths are at most `chunk`: a counting sort
  // (one bucket per length, buckets walked from the longest down) instead of a comparison sort of ~500 k items.
  const size_t n_it = item_row.size();
  std::vector<long> order(n_it);
  static const int order_mode = getenv("CUMF_ALS_ORDER") ? atoi(getenv("CUMF_ALS_ORDER")) : 0;
  // Round 6: whole rows of at most kShortRow ratings go behind everything else (longest first among themselves): the CG of
  // als_short.hip takes exactly the last n_short items of a launch; every other kernel treats items independently.
  long n_short = 0;
  if (order_mode == 0) {
    auto bucket = [&](size_t i) -> size_t {
      const bool is_short = item_slot[i] < 0 && item_len[i] <= kShortRow;
      return is_short ? (size_t)chunk + 1 + (size_t)(kShortRow - item_len[i]) : (size_t)(chunk - item_len[i]);
    };
    std::vector<long> start((size_t)chunk + kShortRow + 3, 0);
    for (size_t i = 0; i < n_it; ++i) {
      ++start[bucket(i) + 1];  // bucket 0 = the longest
      n_short += item_slot[i] < 0 && item_len[i] <= kShortRow;
    }
    for (size_t k = 1; k < start.size(); ++k) start[k] += start[k - 1];
    for (size_t i = 0; i < n_it; ++i) order[(size_t)start[bucket(i)]++] = (long)i;  // stable
  } else {
    std::iota(order.begin(), order.end(), 0L);
  }

  cumf_plan* p = new cumf_plan();
  p->rows = rows;
  p->row_begin = row_begin;
  p->row_end = row_end;
  p->f = f;
  p->nb = nb_for_f(f);
  p->chunk = chunk;
  p->plan_nnz = rp(row_end) - rp(row_begin);
  p->n_items = (long)n_it;
  p->n_short = n_short;
  p->n_slots = n_slots;
  p->n_mrows = (long)mrow_row.size();
  for (size_t i = 0; i < n_it; ++i) {
    if (item_slot[i] >= 0) {
      ++p->n_citems;
      p->chunk_nnz += item_len[i];
    }
  }
  p->n_witems = p->n_items - p->n_citems;
  *out = nullptr;

  // ONE device block and ONE upload for the 19 index arrays (a hipMalloc + a synchronous hipMemcpy each cost more than
  // building the lists: 4 plans x 19 arrays were 40 % of doALS's set-up at the Netflix shape).  256-byte aligned pieces.
  const size_t ni = n_it, nm = mrow_row.size(), nc = (size_t)p->n_citems, nw = (size_t)p->n_witems;
  size_t off = 0;
  auto piece = [&](size_t count, size_t elem) {
    const size_t at = off;
    off += (count * elem + 255) & ~(size_t)255;
    return at;
  };
  const size_t o_item_row = piece(ni, 4), o_item_begin = piece(ni, 8), o_item_len = piece(ni, 4), o_item_slot = piece(ni, 4),
               o_item_rowlen = piece(ni, 4), o_mrow_row = piece(nm, 4), o_mrow_slot0 = piece(nm, 4),
               o_mrow_nslots = piece(nm, 4), o_mrow_rowlen = piece(nm, 4), o_c_row = piece(nc, 4), o_c_begin = piece(nc, 8),
               o_c_len = piece(nc, 4), o_c_slot = piece(nc, 4), o_c_rowlen = piece(nc, 4), o_w_row = piece(nw, 4),
               o_w_begin = piece(nw, 8), o_w_len = piece(nw, 4), o_w_rowlen = piece(nw, 4);
  std::vector<char> host(off ? off : 256);
  auto ints = [&](size_t o) { return reinterpret_cast<int*>(host.data() + o); };
  auto longs = [&](size_t o) { return reinterpret_cast<long long*>(host.data() + o); };
  {
    size_t ic = 0, iw = 0;
    for (size_t k = 0; k < ni; ++k) {  // the sorted order carries over to both sub-lists
      const size_t i = (size_t)order[k];
      ints(o_item_row)[k] = item_row[i];
      longs(o_item_begin)[k] = item_begin[i];
      ints(o_item_len)[k] = item_len[i];
      ints(o_item_slot)[k] = item_slot[i];
      ints(o_item_rowlen)[k] = item_rowlen[i];
      if (item_slot[i] >= 0) {
        ints(o_c_row)[ic] = item_row[i];
        longs(o_c_begin)[ic] = item_begin[i];
        ints(o_c_len)[ic] = item_len[i];
        ints(o_c_slot)[ic] = item_slot[i];
        ints(o_c_rowlen)[ic] = item_rowlen[i];
        ++ic;
      } else {
        ints(o_w_row)[iw] = item_row[i];
        longs(o_w_begin)[iw] = item_begin[i];
        ints(o_w_len)[iw] = item_len[i];
        ints(o_w_rowlen)[iw] = item_rowlen[i];
        ++iw;
      }
    }
    for (size_t k = 0; k < nm; ++k) {
      ints(o_mrow_row)[k] = mrow_row[k];
      ints(o_mrow_slot0)[k] = mrow_slot0[k];
      ints(o_mrow_nslots)[k] = mrow_nslots[k];
      ints(o_mrow_rowlen)[k] = mrow_rowlen[k];
    }
  }
#define PLAN_CHECK(call)                                                                                    \
  do {                                                                                                      \
    hipError_t err__ = (call);                                                                              \
    if (err__ != hipSuccess) {                                                                              \
      fprintf(stderr, "HIP Error:\nFile = %s\nLine = %d\nReason = %s\n", __FILE__, __LINE__,              \
              hipGetErrorString(err__));                                                                    \
      cumf_plan_destroy(p); /* no half-built plan, no leaked device buffers */                             \
      return (int)err__;                                                                                    \
    }                                                                                                       \
  } while (0)
  PLAN_CHECK(hipMalloc(reinterpret_cast<void**>(&p->d_block), host.size()));
  PLAN_CHECK(hipMemcpy(p->d_block, host.data(), host.size(), hipMemcpyHostToDevice));
  auto dints = [&](size_t o, size_t count) { return count ? reinterpret_cast<int*>(p->d_block + o) : nullptr; };
  auto dlongs = [&](size_t o, size_t count) { return count ? reinterpret_cast<long long*>(p->d_block + o) : nullptr; };
  p->d_item_row = dints(o_item_row, ni), p->d_item_begin = dlongs(o_item_begin, ni), p->d_item_len = dints(o_item_len, ni);
  p->d_item_slot = dints(o_item_slot, ni), p->d_item_rowlen = dints(o_item_rowlen, ni);
  p->d_mrow_row = dints(o_mrow_row, nm), p->d_mrow_slot0 = dints(o_mrow_slot0, nm);
  p->d_mrow_nslots = dints(o_mrow_nslots, nm), p->d_mrow_rowlen = dints(o_mrow_rowlen, nm);
  p->d_c_row = dints(o_c_row, nc), p->d_c_begin = dlongs(o_c_begin, nc), p->d_c_len = dints(o_c_len, nc);
  p->d_c_slot = dints(o_c_slot, nc), p->d_c_rowlen = dints(o_c_rowlen, nc);
  p->d_w_row = dints(o_w_row, nw), p->d_w_begin = dlongs(o_w_begin, nw), p->d_w_len = dints(o_w_len, nw);
  p->d_w_rowlen = dints(o_w_rowlen, nw);
  if (n_slots > 0) {
    const size_t tiles = (size_t)p->nb * (p->nb + 1) / 2;
    PLAN_CHECK(hipMalloc(reinterpret_cast<void**>(&p->d_part), (size_t)n_slots * tiles * 256 * sizeof(float)));
  }
#undef PLAN_CHECK
  *out = p;
  return 0;
}

extern "C" int cumf_plan_destroy(cumf_plan_t* p) {
  if (!p) return 0;
  if (p->d_block) (void)hipFree(p->d_block);  // every index array lives in this one block
  if (p->d_part) (void)hipFree(p->d_part);
  free_implicit_lists(p->implicit);
  delete p;
  return 0;
}

extern "C" int cumf_plan_set_gather_rows(cumf_plan_t* p, long gather_rows) {
  if (!p || gather_rows < 0) return (int)hipErrorInvalidValue;
  p->gather_rows = gather_rows;
  return 0;
}

extern "C" int cumf_plan_info(const cumf_plan_t* p, long info[4]) {
  if (!p || !info) return (int)hipErrorInvalidValue;
  info[0] = p->n_items;
  info[1] = p->n_slots;
  info[2] = p->n_mrows;
  info[3] = p->chunk;
  return 0;
}

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

namespace {

int fast_flag_get(int** out) {
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

// Work lists of a plan for launch_half_iteration; need_tiles: the dense-slot tile buffer (Route::whole == kSolveTileBuffer).
int plan_lists(const cumf_plan_t* p, PlanLists* out, hipStream_t stream, bool need_tiles) {
  const size_t tile_bytes = (size_t)p->nb * (p->nb + 1) / 2 * 256 * sizeof(float);
  float* part2 = nullptr;
  long rows = 0;
  if (need_tiles && p->n_witems > 0) {
    // Sized for 288 GB of HBM: up to 48 GiB (CUMF_ALS_TILE_BUFFER_GB), never more than half of what is free -- the
    // Netflix Theta side at f = 200 (480 189 rows x 93 KB = 44.7 GB) then runs as ONE Gram launch + ONE LU launch
    // instead of 21 pairs of 2 GiB batches, each with its own tail.
    static const double cap_gb = getenv("CUMF_ALS_TILE_BUFFER_GB") ? atof(getenv("CUMF_ALS_TILE_BUFFER_GB")) : 48.0;
    size_t cap = (size_t)(cap_gb * (double)(1ull << 30));
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
      std::lock_guard<std::mutex> lock(g_scratch_mutex);
      int dev = 0;
      (void)hipGetDevice(&dev);
      auto have = g_scratch.find(std::make_tuple(dev, stream, kScratchTiles));
      const size_t mine = have != g_scratch.end() ? have->second.cap : 0;  // our own buffer counts as available
      cap = std::min(cap, (free_b + mine) / 2);
    }
    if (cap < ((size_t)2 << 30)) cap = (size_t)2 << 30;
    rows = (long)std::min<size_t>((size_t)p->n_witems, cap / tile_bytes);
    if (rows < 1) rows = 1;
    void* q = nullptr;
    const int rc = scratch_get(stream, kScratchTiles, (size_t)rows * tile_bytes, &q);
    if (rc) return rc;
    part2 = static_cast<float*>(q);
  }
  *out = PlanLists{p->n_items,  p->n_mrows, p->n_citems, p->n_witems, p->d_c_row,    p->d_c_len,  p->d_c_slot,
                   p->d_c_rowlen, p->d_c_begin, p->d_w_row,  p->d_w_len,  p->d_w_rowlen, p->d_w_begin, part2,
                   rows,          p->plan_nnz > 0 ? (double)p->chunk_nnz / (double)p->plan_nnz : 0.0, p->n_short};
  return 0;
}

#if CUMF_ABLATE
// Ablation switches of the kernels, profiling build only (libALS_ablate.so; CUMF_ALS_DBG /
// cumf_set_debug_switches): any value but 0 makes the results wrong on purpose -- 1 = no solve, 2 = no Gram
// pass, 8 = every gather hits row 0, 16 = no gather DMA.
int g_debug_switches = -1;
int debug_switches() {
  if (g_debug_switches < 0) g_debug_switches = getenv("CUMF_ALS_DBG") ? atoi(getenv("CUMF_ALS_DBG")) : 0;
  return g_debug_switches;
}
#endif

KernelArgs base_args(const cumf_plan_t* p, const int* colidx, const float* val, const float* gather, int f,
                     float lambda) {
  KernelArgs a{};
  a.item_row = p->d_item_row;
  a.item_begin = p->d_item_begin;
  a.item_len = p->d_item_len;
  a.item_slot = p->d_item_slot;
  a.item_rowlen = p->d_item_rowlen;
  a.mrow_row = p->d_mrow_row;
  a.mrow_slot0 = p->d_mrow_slot0;
  a.mrow_nslots = p->d_mrow_nslots;
  a.mrow_rowlen = p->d_mrow_rowlen;
  a.part = p->d_part;
  a.colidx = colidx;
  a.val = val;
  a.gather = gather;
  a.gather_f32 = gather;
  a.row_begin = p->row_begin;
  a.f = f;
  a.lambda = lambda;
#if CUMF_ABLATE
  a.dbg = debug_switches();
#endif
  return a;
}

// Gram mode "fast": the factor table as (h, l) f16 words, rebuilt per call (the factors change every
// half-iteration: 2 x 192 MB of traffic for the Netflix X table, ~0.1 ms).
int fast_words(const cumf_plan_t* p, const float* gather, int f, hipStream_t stream, KernelArgs* a) {
  if (p->gather_rows <= 0) {
    fprintf(stderr, "cumf_als_update_fused: gram mode \"fast\" needs the row count of the gather table "
                    "(cumf_plan_set_gather_rows)\n");
    return (int)hipErrorInvalidValue;
  }
  const size_t n = (size_t)p->gather_rows * f;
  void* words = nullptr;
  int rc = scratch_get(stream, kScratchWords, n * sizeof(unsigned), &words);
  if (rc) return rc;
  int* flag = nullptr;
  rc = fast_flag_get(&flag);
  if (rc) return rc;
  CUMF_HIP_CHECK(launch_presplit(gather, static_cast<unsigned*>(words), n, flag, stream));
  a->gather = reinterpret_cast<const float*>(words);
  a->fast_flag = flag;
  return 0;
}

// Round 6 (kArithPre): the gather table as bf16 h | m | l planes, rebuilt per call (als_route.cpp: presplit_wanted).
int pre_words(const cumf_plan_t* p, const float* gather, int f, hipStream_t stream, KernelArgs* a) {
  void* planes = nullptr;
  const int rc = scratch_get(stream, kScratchPlanes, (size_t)p->gather_rows * presplit_pitch(f), &planes);
  if (rc) return rc;
  CUMF_HIP_CHECK(launch_presplit3(gather, planes, p->gather_rows, f, stream));
  a->gather = reinterpret_cast<const float*>(planes);
  a->pre_pitch = presplit_pitch(f);
  return 0;
}

PlanFacts plan_facts(const cumf_plan_t* p) {
  return PlanFacts{p->nb, p->n_mrows, p->n_citems, p->n_witems,
                   p->plan_nnz > 0 ? (double)p->chunk_nnz / (double)p->plan_nnz : 0.0, p->n_short, p->gather_rows};
}

thread_local int g_last_error = 0;  // per host thread: concurrent doALS calls do not see each other's state

}  // namespace

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

// Error state of the entry points that return a value instead of a code (cumf_doALS_ex returns NaN and sets
// this): 0 = none, otherwise a HIP error code or one of CUMF_ERR_*.  Reading clears it.
extern "C" int cumf_last_error(void) {
  const int e = g_last_error;
  g_last_error = 0;
  return e;
}
void cumf::set_last_error(int code) { g_last_error = code; }

// Demangled name of the Gram(+solve) kernel the last half-iteration of this process dispatched, as a profiler
// prints it (e.g. "cumf::als_wave_kernel<7, 1, 100, 0>"); empty before the first launch.
extern "C" int cumf_last_kernel_name(char* buf, int cap) {
  if (!buf || cap <= 0) return (int)hipErrorInvalidValue;
  buf[0] = 0;
  const void* fn = last_item_kernel();
  if (!fn) return 0;
  const char* mangled = hipKernelNameRefByPtr(fn, nullptr);
  if (!mangled) return 0;
  int status = 0;
  char* dem = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
  const char* name = (status == 0 && dem) ? dem : mangled;
  size_t len = strlen(name);
  // drop the parameter list -- the first '(' outside the template brackets ("float __vector(4)" is a template
  // argument of the workgroup kernels) -- and the "void " of a template instance
  int depth = 0;
  for (size_t i = 0; name[i]; ++i) {
    if (name[i] == '<') ++depth;
    if (name[i] == '>') --depth;
    if (name[i] == '(' && depth == 0) {
      len = i;
      break;
    }
  }
  if (strncmp(name, "void ", 5) == 0) {
    name += 5;
    len -= 5;
  }
  if (len >= (size_t)cap) len = (size_t)cap - 1;
  memcpy(buf, name, len);
  buf[len] = 0;
  free(dem);
  return 0;
}

// Can one fused call (RHS + Gram + solve) handle (f, solver)?  Even f with a route (route_for, als_route.cpp).
extern "C" int cumf_fused_available(int f, int solver) {
  const int mode = solver == CUMF_SOLVER_LU ? kModeLU : kModeCG;
  if (f <= 0 || (f % 2) != 0 || (solver != CUMF_SOLVER_CG && solver != CUMF_SOLVER_LU)) return 0;
  return route_for(f, mode, PlanFacts{}, switches()).path != kPathNone;
}

namespace {
int update_fused_impl(const cumf_plan_t* p, const int* colidx, const float* val, const float* gather, float* update, int f,
                      float lambda, int solver, int cg_iters, double* sse_bins, void* stream) {
  if (!p || f != p->f) {
    fprintf(stderr, "cumf_als_update_fused: plan/f mismatch\n");
    return (int)hipErrorInvalidValue;
  }
  if (!cumf_fused_available(f, solver)) {
    fprintf(stderr, "cumf_als_update_fused: f = %d with this solver needs the materialising path "
                    "(cumf_get_hermitian + cumf_*_solve_batched): the fused CG holds the full system "
                    "in LDS (f <= 128), the fused LU its packed upper triangle (f <= 200)\n", f);
    return (int)hipErrorInvalidValue;
  }
  ScratchLease lease;  // pooled tile buffer / pre-split table stay ours until the last launch below is enqueued
  KernelArgs a = base_args(p, colidx, val, gather, f, lambda);
  a.update = update;
  a.cg_iters = cg_iters;
  a.sse_bins = sse_bins;
  const int mode = (solver == CUMF_SOLVER_LU) ? kModeLU : kModeCG;
  const Route r = route_for(f, mode, plan_facts(p), switches());
  PlanLists lists{};
  int rc = plan_lists(p, &lists, static_cast<hipStream_t>(stream), r.whole == kSolveTileBuffer);
  if (!rc && r.table == kTableF16Words) rc = fast_words(p, gather, f, static_cast<hipStream_t>(stream), &a);
  if (!rc && r.table == kTablePlanes) rc = pre_words(p, gather, f, static_cast<hipStream_t>(stream), &a);
  if (rc) return rc;
  CUMF_HIP_CHECK(launch_half_iteration(a, mode, r, lists, static_cast<hipStream_t>(stream)));
  return 0;
}
}  // namespace

extern "C" int cumf_als_update_fused(const cumf_plan_t* p, const int* colidx, const float* val, const float* gather,
                                     float* update, int f, float lambda, int solver, int cg_iters, void* stream) {
  return update_fused_impl(p, colidx, val, gather, update, f, lambda, solver, cg_iters, nullptr, stream);
}

// Can the half-iteration of this plan also deliver the train SSE of its rows (cumf_als_update_fused_sse)?  Where every
// solver on its route adds it (Route::sse; route_for spells out the two gaps).
extern "C" int cumf_fused_sse_available(const cumf_plan_t* p, int solver) {
  if (!p || (solver != CUMF_SOLVER_CG && solver != CUMF_SOLVER_LU)) return 0;
  return route_for(p->f, solver == CUMF_SOLVER_LU ? kModeLU : kModeCG, plan_facts(p), switches()).sse;
}

// cumf_als_update_fused + the train SSE of the updated rows for free (als.cu:979-991 folded into the update, see
// wave_tile_ff in als_wave.hip): sum over the plan's rows of sum_u (r - x_u . t)^2 is ADDED, spread over the
// CUMF_SSE_BINS fp64 words of sse_bins (device memory, zeroed by the caller; the total is their sum).
extern "C" int cumf_als_update_fused_sse(const cumf_plan_t* p, const int* colidx, const float* val, const float* gather,
                                         float* update, int f, float lambda, int solver, int cg_iters, double* sse_bins,
                                         void* stream) {
  if (!sse_bins || !cumf_fused_sse_available(p, solver)) {
    fprintf(stderr, "cumf_als_update_fused_sse: not available for this plan (cumf_fused_sse_available)\n");
    return (int)hipErrorInvalidValue;
  }
  return update_fused_impl(p, colidx, val, gather, update, f, lambda, solver, cg_iters, sse_bins, stream);
}

namespace {
// storage: 0 = fp32 f x f (both triangles), 1 = fp16 f x f, 2 = fp32 packed upper triangle
int get_hermitian_any(const char* who, const cumf_plan_t* p, const int* colidx, const float* val, const float* gather,
                      void* tt, float* rhs, int f, float lambda, void* stream, int storage) {
  if (!p || f != p->f) {
    fprintf(stderr, "%s: plan/f mismatch\n", who);
    return (int)hipErrorInvalidValue;
  }
  ScratchLease lease;
  KernelArgs a = base_args(p, colidx, val, gather, f, lambda);
  a.tt = static_cast<float*>(tt);
  a.tt_half = storage == 1;
  a.tt_packed = storage == 2;
  a.rhs = rhs;
  const Route r = route_for(f, kModeMaterialize, plan_facts(p), switches());
  if (r.path == kPathGeneric) {  // above the tile kernels' range: the plain kernel of als_generic.hip, fp32 f x f storage only
    if (storage != 0) {
      fprintf(stderr, "%s: f = %d is above the tile kernels' range (%d): only the fp32 f x f batch (cumf_get_hermitian)\n", who, f, kMaxF);
      return (int)hipErrorInvalidValue;
    }
    CUMF_HIP_CHECK(launch_gram_generic(a, p->n_items, static_cast<hipStream_t>(stream)));
    return 0;
  }
  PlanLists lists{};
  const int rc = plan_lists(p, &lists, static_cast<hipStream_t>(stream), r.whole == kSolveTileBuffer);
  if (rc) return rc;
  CUMF_HIP_CHECK(launch_half_iteration(a, kModeMaterialize, r, lists, static_cast<hipStream_t>(stream)));
  return 0;
}
}  // namespace

extern "C" int cumf_get_hermitian(const cumf_plan_t* p, const int* colidx, const float* val, const float* gather,
                                  float* tt, float* rhs, int f, float lambda, void* stream) {
  return get_hermitian_any("cumf_get_hermitian", p, colidx, val, gather, tt, rhs, f, lambda, stream, 0);
}

extern "C" int cumf_get_hermitian_fp16(const cumf_plan_t* p, const int* colidx, const float* val, const float* gather,
                                       void* tt_half, float* rhs, int f, float lambda, void* stream) {
  return get_hermitian_any("cumf_get_hermitian_fp16", p, colidx, val, gather, tt_half, rhs, f, lambda, stream, 1);
}

// The Gram batch as packed upper triangles, written straight from the accumulators: what the multi-GPU
// Theta phase reduces across GPUs (hugewiki.cu:2703-2717 moves full f x f matrices) -- no f x f batch is
// materialised and no pack pass runs.
extern "C" int cumf_get_hermitian_packed(const cumf_plan_t* p, const int* colidx, const float* val,
                                         const float* gather, float* packed, float* rhs, int f, float lambda,
                                         void* stream) {
  return get_hermitian_any("cumf_get_hermitian_packed", p, colidx, val, gather, packed, rhs, f, lambda, stream, 2);
}

extern "C" int cumf_cg_solve_batched_fp16(const void* A_half, float* x, const float* b, long batch, int f,
                                          int cg_iters, void* stream) {
  if (f <= 0 || f > 256) return (int)hipErrorInvalidValue;
  CUMF_HIP_CHECK(launch_solve_batched(static_cast<const float*>(A_half), b, x, batch, f, kModeCGHalf, cg_iters,
                                      static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int cumf_cg_solve_batched(const float* A, float* x, const float* b, long batch, int f, int cg_iters,
                                     void* stream) {
  if (f <= 0 || f > kMaxFAny) return (int)hipErrorInvalidValue;  // above f = 128: cg_global_kernel, one thread per row of the system
  CUMF_HIP_CHECK(launch_solve_batched(A, b, x, batch, f, kModeCG, cg_iters, static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int cumf_lu_solve_batched(const float* A, const float* b, float* x, long batch, int f, void* stream) {
  if (f <= 0 || f > kMaxFAny) {
    fprintf(stderr, "cumf_lu_solve_batched: f = %d unsupported (f <= %d)\n", f, kMaxFAny);
    return (int)hipErrorInvalidValue;
  }
  if (f > 200) {
    // above the LDS-resident solvers: the elimination in global memory, in the operation order of the unpivoted Doolittle LU +
    // getrs (als_generic.hip).  A is overwritten with the factors, as cublasSgetrfBatched overwrites it (als.cu:77).
    CUMF_HIP_CHECK(launch_lu_global(const_cast<float*>(A), b, x, batch, f, static_cast<hipStream_t>(stream)));
    return 0;
  }
  // CUMF_ALS_LU_EXACT=1: the LDS-resident elimination in the oracle's exact operation order
  // (bit-identical to oracle_lu); default: the register-resident symmetric elimination.
  const int mode = switches().lu_exact ? kModeLUExact : kModeLU;
  CUMF_HIP_CHECK(launch_solve_batched(A, b, x, batch, f, mode, 0, static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int cumf_pack_upper(const float* full, float* packed, long batch, int f, void* stream) {
  CUMF_HIP_CHECK(launch_pack_upper(full, packed, batch, f, 0, static_cast<hipStream_t>(stream)));
  return 0;
}
extern "C" int cumf_unpack_upper(const float* packed, float* full, long batch, int f, void* stream) {
  CUMF_HIP_CHECK(launch_pack_upper(packed, full, batch, f, 1, static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int cumf_sse(const float* val, const int* row, const int* col, const float* thetaT, const float* XT,
                        long count, int f, int surpass_nan, double* sse_out, void* stream) {
  CUMF_HIP_CHECK(launch_sse(val, row, col, thetaT, XT, count, f, surpass_nan, sse_out, static_cast<hipStream_t>(stream)));
  return 0;
}

// Train SSE from materialised systems: *sse_terms += sum over the batch of 2 x.b - x^T A x + reg[v] |x|^2 (fp64), so that
// sum_u (r - x_u . t)^2 over the batch's ratings = (their sum r^2) - that.  A: batch x f x f (symmetric, reg[v] = lambda n_v
// on the diagonal), b, x: batch x f, reg: batch floats; a system without ratings is marked by reg < 0 and skipped.
extern "C" int cumf_quadratic_sse_terms(const float* A, const float* b, const float* x, const float* reg, long batch, int f,
                                        double* sse_terms, void* stream) {
  if (!A || !b || !x || !reg || !sse_terms) return (int)hipErrorInvalidValue;
  CUMF_HIP_CHECK(launch_quadratic_terms(A, b, x, reg, batch, f, sse_terms, static_cast<hipStream_t>(stream)));
  return 0;
}

// The workgroup-per-item kernels (als_kernels.hip) address the gather table with 32-bit byte offsets
// (Stager::gather_pass); the wave-per-item kernels use 64-bit lane addresses.  Fail loudly instead of
// gathering garbage (VERDICT r01 / ADVICE r01: hugewiki X on one GPU is 20 GB).
extern "C" int cumf_check_gather_table(long gather_rows, int f, int solver, int materialize) {
  const int mode = materialize ? kModeMaterialize : (solver == CUMF_SOLVER_LU ? kModeLU : kModeCG);
  if (gather_rows < 0 || f <= 0) return (int)hipErrorInvalidValue;
  if (solver != CUMF_SOLVER_CG && solver != CUMF_SOLVER_LU) {
    fprintf(stderr, "cumf_als: solver %d is not an explicit-feedback solver (CUMF_SOLVER_CG or CUMF_SOLVER_LU)\n", solver);
    return (int)hipErrorInvalidValue;
  }
  if (f > kMaxF) return 0;  // als_generic.hip: 64-bit gather addresses
  const Path path = route_for(f, mode, PlanFacts{}, switches()).path;
  if (path == kPathOneWave || path == kPathTwoWave) return 0;  // the wave kernels: 64-bit addresses too
  const unsigned long long bytes = (unsigned long long)gather_rows * (unsigned long long)f * 4ull;
  if (bytes >= (1ull << 32)) {
    fprintf(stderr,
            "cumf_als: the gathered factor table is %llu bytes (%ld rows x f = %d); this solver / f combination "
            "runs the kernels with 32-bit gather offsets (limit 4 GiB).  Shard the gathered side (cumf_als_amd.dist) "
            "or use the LU solver with f <= %d (64-bit addressing).\n",
            bytes, gather_rows, f, 16 * kMaxWaveNB - 1);
    return (int)hipErrorInvalidValue;
  }
  return 0;
}

extern "C" int cumf_set_gram_mode(int mode) {
  if (mode != CUMF_GRAM_AUTO && mode != CUMF_GRAM_EXACT && mode != CUMF_GRAM_FAST) return (int)hipErrorInvalidValue;
  set_gram_mode(mode);
  return 0;
}
extern "C" int cumf_get_gram_mode(void) { return switches().gram; }

extern "C" int cumf_set_presplit(int mode) {
  if (mode != CUMF_PRESPLIT_AUTO && mode != CUMF_PRESPLIT_OFF && mode != CUMF_PRESPLIT_ON && mode != CUMF_PRESPLIT_VERIFY)
    return (int)hipErrorInvalidValue;
  set_presplit_mode(mode);
  return 0;
}
extern "C" int cumf_get_presplit(void) { return switches().presplit; }
extern "C" long cumf_presplit_pitch(int f) { return presplit_supported(f) ? (long)presplit_pitch(f) : 0; }
extern "C" int cumf_presplit_table(const float* table, void* planes, long rows, int f, void* stream) {
  if (!table || !planes || rows < 0 || !presplit_supported(f)) return (int)hipErrorInvalidValue;
  CUMF_HIP_CHECK(launch_presplit3(table, planes, rows, f, static_cast<hipStream_t>(stream)));
  return 0;
}

#if CUMF_ABLATE
// profiling build only (not declared in include/): see debug_switches() above
extern "C" int cumf_set_debug_switches(int switches) {
  if (switches < 0) return (int)hipErrorInvalidValue;
  g_debug_switches = switches;
  return 0;
}
// switch 65536: rows by the number of CG iterations they ran (bins 0 .. 15), read and cleared; f selects the kernels'
// feature-block count (the profiling build has NB = 5, 7, 13)
extern "C" int cumf_debug_cg_histogram(int f, unsigned long long* out16) {
  if (!out16) return (int)hipErrorInvalidValue;
  CUMF_HIP_CHECK(hipDeviceSynchronize());
  switch (nb_for_f(f)) {
    case 5: CUMF_HIP_CHECK(cumf::wave_cg_hist<5>(out16)); break;
    case 7: CUMF_HIP_CHECK(cumf::wave_cg_hist<7>(out16)); break;
    case 13: CUMF_HIP_CHECK(cumf::wave_cg_hist<13>(out16)); break;
    default: return (int)hipErrorInvalidValue;
  }
  return 0;
}
#endif

extern "C" int cumf_set_kernel_timing(int enable) {
  set_kernel_timing(enable != 0);
  return 0;
}

extern "C" int cumf_last_kernel_ms(float* item_kernel_ms, float* reduce_kernel_ms) {
  if (!item_kernel_ms || !reduce_kernel_ms) return (int)hipErrorInvalidValue;
  CUMF_HIP_CHECK(last_kernel_ms(item_kernel_ms, reduce_kernel_ms));
  return 0;
}

extern "C" int cumf_kernel_ms_since_reset(float* item_kernel_ms, float* reduce_kernel_ms, int* launches) {
  if (!item_kernel_ms || !reduce_kernel_ms || !launches) return (int)hipErrorInvalidValue;
  CUMF_HIP_CHECK(kernel_ms_since_reset(item_kernel_ms, reduce_kernel_ms, launches));
  return 0;
}

extern "C" void cumf_rand_init(float* a, long count, float scale, long seed) {
  if (seed >= 0) srand((unsigned)seed);
  for (long k = 0; k < count; ++k) a[k] = scale * ((float)rand() / (float)RAND_MAX);
}

extern "C" int cumf_als_version(void) { return 100; }
extern "C" const char* cumf_als_arch(void) { return "gfx950"; }

// cg.h:32, cg.cu:641-644: A holds halves (the reference casts the float* it is handed: `(half*)A`)
void updateXWithCGHost_tt_fp16(float* A, float* x, float* b, const int batchSize, const int f, const float cgIter) {
  int rc = cumf_cg_solve_batched_fp16(A, x, b, batchSize, f, (int)ceilf(cgIter), nullptr);
  hipError_t e = hipDeviceSynchronize();
  if (rc != 0 || e != hipSuccess) {
    fprintf(stderr, "updateXWithCGHost_tt_fp16 failed: %s\n", hipGetErrorString(rc ? (hipError_t)rc : e));
    exit(EXIT_FAILURE);
  }
}

// C++-linkage drop-in of the reference's inner solver API (cg.h:30, cg.cu:682-686):
// device pointers, synchronous, aborts on error like cudaCheckError (als.h:667-674).
void updateXWithCGHost(float* A, float* x, float* b, const int batchSize, const int f, const float cgIter) {
  int rc = cumf_cg_solve_batched(A, x, b, batchSize, f, (int)ceilf(cgIter), nullptr);
  hipError_t e = hipDeviceSynchronize();
  if (rc != 0 || e != hipSuccess) {
    fprintf(stderr, "updateXWithCGHost failed: %s\n", hipGetErrorString(rc ? (hipError_t)rc : e));
    exit(EXIT_FAILURE);
  }
}

// C++-linkage drop-in of the reference's fused Gram + CG host (cg.h:34-36, cg.cu:1190-1197; disabled at its only
// call site, als.cu:809-812: "performance not good").  DEVICE pointers, synchronous.  For the rows
// batch_offset .. m - 1 of the CSR matrix: A = sum theta theta^T + lambda * n_row * I over the row's columns
// (cg.cu:735-840), then cgIter warm-started CG steps on A x = ythetaT with x = XT (cg.cu:826-1186).  XT and
// ythetaT are BATCH-LOCAL: system b (row batch_offset + b) uses XT[b * F ...] and ythetaT[b * F ...].  (The
// reference kernel strides ythetaT by blockDim.x = 64 instead of F, cg.cu:941 -- a defect of the disabled
// code path that is not reproduced -- and hard-codes F = 100 in its loader; any f the library supports works
// here.)  The ratings themselves are not an argument (the right-hand side comes precomputed), so the Gram
// batch is formed with the materialising kernels, at most 4 GiB at a time, and handed to the batched CG.
void alsUpdateFeature100Host(const int batch_offset, const int* csrRowIndex, const int* csrColIndex,
                             const float lambda, const int m, const int F, const float* thetaT, float* XT,
                             float* ythetaT, int cgIter) {
  auto fail = [](const char* what, int code) {
    fprintf(stderr, "alsUpdateFeature100Host failed (%s): %s\n", what, hipGetErrorString((hipError_t)code));
    exit(EXIT_FAILURE);
  };
  if (batch_offset < 0 || m < 0 || !csrRowIndex || !csrColIndex || !thetaT || !XT || !ythetaT)
    fail("arguments", (int)hipErrorInvalidValue);
  const long rows = (long)m - batch_offset;
  if (rows <= 0) return;
  std::vector<int> rowptr((size_t)m + 1);
  hipError_t e = hipMemcpy(rowptr.data(), csrRowIndex, rowptr.size() * sizeof(int), hipMemcpyDeviceToHost);
  if (e != hipSuccess) fail("row pointer", (int)e);
  // 2^31 or more ratings: the 4-byte row pointer has wrapped (hugewiki.cu:1973 reads it as unsigned): widen it; a row
  // pointer that is not non-decreasing as unsigned values is rejected by the plan (negative row lengths)
  std::vector<long long> rowptr64((size_t)m + 1);
  {
    long long hi = 0;
    unsigned prev = (unsigned)rowptr[0];
    rowptr64[0] = prev;
    for (long i = 1; i <= m; ++i) {
      const unsigned cur = (unsigned)rowptr[(size_t)i];
      if (cur < prev) hi += 1ll << 32;
      rowptr64[(size_t)i] = hi + cur;
      prev = cur;
    }
  }
  // the rating slot of the gathered rows (the fused right-hand side) reads zeros: this entry point has no ratings
  // (val == nullptr: the kernels read their zero row instead)
  const size_t sys_bytes = (size_t)F * F * sizeof(float);
  const long per_batch = std::max<long>(1, (long)(((size_t)4 << 30) / sys_bytes));
  float* tt = nullptr;
  if ((e = hipMalloc(reinterpret_cast<void**>(&tt), (size_t)std::min(rows, per_batch) * sys_bytes)) != hipSuccess)
    fail("Gram batch", (int)e);
  for (long b0 = 0; b0 < rows; b0 += per_batch) {
    const long nb = std::min(per_batch, rows - b0);
    cumf_plan_t* plan = nullptr;
    int rc = cumf_plan_create(&plan, rowptr64.data(), 1, m, batch_offset + b0, batch_offset + b0 + nb, F, 0);
    if (rc) fail("plan", rc);
    rc = cumf_get_hermitian(plan, csrColIndex, nullptr, thetaT, tt, nullptr, F, lambda, nullptr);
    if (rc) fail("Gram", rc);
    rc = cumf_cg_solve_batched(tt, XT + (size_t)b0 * F, ythetaT + (size_t)b0 * F, nb, F, cgIter, nullptr);
    if (rc) fail("CG", rc);
    if ((e = hipDeviceSynchronize()) != hipSuccess) fail("kernels", (int)e);
    cumf_plan_destroy(plan);
  }
  (void)hipFree(tt);
}
