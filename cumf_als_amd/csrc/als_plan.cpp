// als_plan.cpp -- static work decomposition of one ALS half-iteration (the cumf_plan_* entry points of
// include/cumf_als_capi.h) and what the other entry points take from a plan (plan_lists, plan_facts).
//
// The reference launches one CUDA block per row (als.cu:449) inside a per-batch loop
// (als.cu:768-777, 881-890).  On the Netflix X side that is 17 770 rows with up to
// ~230k ratings each over 256 CUs: the tail row alone would run for milliseconds.
// The plan cuts every row into chunks of at most `chunk` ratings ("items"), orders
// the items longest-first and gives each chunk of a split row a slot in a partial
// tile buffer that the reduce kernel sums in slot order (deterministic).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "als_internal.h"
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

// Whole rows (at most `chunk` ratings) of [row_begin, row_end) by length: 1 .. kDualMaxRow, 1 .. kDualMaxRow6, none.  A row's
// own length decides, so the batched plans of one side count what the unbatched plan counts.
template <class RP>
void count_dual_rows(const RP& rp, long row_begin, long row_end, int chunk, long* n_dual, long* n_dual6, long* n_empty) {
  *n_dual = *n_dual6 = *n_empty = 0;
  for (long u = row_begin; u < row_end; ++u) {
    const long long len = rp(u + 1) - rp(u);
    if (len > chunk) continue;
    *n_empty += len == 0;
    *n_dual += len >= 1 && len <= kDualMaxRow;
    *n_dual6 += len >= 1 && len <= kDualMaxRow6;
  }
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
  // So do the whole rows of at most kDualMaxRow ratings, in front of them: the dual-form LU (als_dual.hip) takes the items in
  // front of the rows without ratings, in the full list (a combined launch of chunk items and whole rows) as in the
  // whole-row list -- a row is solved the same way whatever else its plan holds.
  long n_short = 0, n_dual = 0, n_dual6 = 0, n_empty = 0;
  if (order_mode == 0) {
    static_assert(kDualMaxRow >= kShortRow, "the short rows are the end of the tail");
    auto bucket = [&](size_t i) -> size_t {
      const bool is_tail = item_slot[i] < 0 && item_len[i] <= kDualMaxRow;
      return is_tail ? (size_t)chunk + 1 + (size_t)(kDualMaxRow - item_len[i]) : (size_t)(chunk - item_len[i]);
    };
    std::vector<long> start((size_t)chunk + kDualMaxRow + 3, 0);
    for (size_t i = 0; i < n_it; ++i) {
      ++start[bucket(i) + 1];  // bucket 0 = the longest
      n_short += item_slot[i] < 0 && item_len[i] <= kShortRow;
    }
    count_dual_rows(rp, row_begin, row_end, chunk, &n_dual, &n_dual6, &n_empty);
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
  p->entry_begin = rp(row_begin);
  p->n_items = (long)n_it;
  p->n_short = n_short;
  p->n_dual = n_dual, p->n_dual6 = n_dual6, p->n_empty = n_empty;
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
  free_seg_lists(p->free_seg);
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

// Rows of the pooled tile buffer for `n_rows` whole rows of `tile_bytes` each: the one place that sizes it.
//   CUMF_ALS_TILE_BUFFER_GB set (read at every call, like CUMF_ALS_LU_EXACT in switches()): that many GiB as given, down to the
//   tiles of one row -- what an operator sets on a card that other work fills, and what makes the batch loop of
//   two_wave_items reachable by a test (tests/test_two_wave_batches_gpu.py).
//   Default: sized for 288 GB of HBM, up to 48 GiB but never more than half of what is free and never below 2 GiB -- the
//   Netflix Theta side at f = 200 (480 189 rows x 93 KB = 44.7 GB) then runs as ONE Gram launch + ONE LU launch instead of
//   21 pairs of 2 GiB batches, each with its own tail.
long tile_buffer_rows(long n_rows, size_t tile_bytes, hipStream_t stream) {
  size_t cap;
  if (const char* e = getenv("CUMF_ALS_TILE_BUFFER_GB")) {
    const double gb = std::min(atof(e), 1048576.0);  // not a number, zero or negative: one row
    cap = gb > 0.0 ? (size_t)(gb * (double)(1ull << 30)) : 0;
  } else {
    cap = (size_t)48 << 30;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
      const size_t mine = scratch_capacity(stream, kScratchTiles);  // our own buffer counts as available
      cap = std::min(cap, (free_b + mine) / 2);
    }
    cap = std::max(cap, (size_t)2 << 30);
  }
  return (long)std::max<size_t>(1, std::min<size_t>((size_t)n_rows, cap / tile_bytes));
}

}  // namespace

// Work lists of a plan for launch_half_iteration; need_tiles: the dense-slot tile buffer (Route::whole == kSolveTileBuffer).
int cumf::plan_lists(const cumf_plan_t* p, PlanLists* out, hipStream_t stream, bool need_tiles) {
  const size_t tile_bytes = (size_t)p->nb * (p->nb + 1) / 2 * 256 * sizeof(float);
  float* part2 = nullptr;
  long rows = 0;
  if (need_tiles && p->n_witems > 0) {
    rows = tile_buffer_rows(p->n_witems, tile_bytes, stream);
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

PlanFacts cumf::plan_facts(const cumf_plan_t* p) {
  return PlanFacts{p->nb, p->n_mrows, p->n_citems, p->n_witems,
                   p->plan_nnz > 0 ? (double)p->chunk_nnz / (double)p->plan_nnz : 0.0, p->n_short, p->gather_rows,
                   p->n_dual, p->n_empty};
}

// Host only (no HIP call, no plan): what a plan of these rows would count for the dual-form route and what the route, with the
// switches as they are now, would hand to it.
extern "C" int cumf_dual_rows_probe(const void* rowptr_host, int rowptr_is_64, long rows, long row_begin, long row_end, int f,
                                    int chunk, int solver, int materialize, long gather_rows, long info[4]) {
  if (!rowptr_host || !info || rows < 0 || row_begin < 0 || row_end > rows || row_begin > row_end || f <= 0 || chunk < kStage)
    return (int)hipErrorInvalidValue;
  auto rp = [&](long i) -> long long {
    return rowptr_is_64 ? static_cast<const long long*>(rowptr_host)[i]
                        : static_cast<long long>(static_cast<const int*>(rowptr_host)[i]);
  };
  chunk = (chunk / kStage) * kStage;
  PlanFacts facts{};
  facts.nb = nb_for_f(f);
  facts.gather_rows = gather_rows;
  long long nnz = 0, chunk_nnz = 0;
  for (long u = row_begin; u < row_end; ++u) {
    const long long len = rp(u + 1) - rp(u);
    nnz += len;
    if (len <= chunk) {
      ++facts.n_witems;
      facts.n_short += len <= kShortRow;
    } else {
      ++facts.n_mrows;
      facts.n_citems += (long)((len + chunk - 1) / chunk);
      chunk_nnz += len;
    }
  }
  facts.chunk_share = nnz > 0 ? (double)chunk_nnz / (double)nnz : 0.0;
  long n_dual6 = 0;
  count_dual_rows(rp, row_begin, row_end, chunk, &facts.n_dual, &n_dual6, &facts.n_empty);
  const int mode = materialize ? kModeMaterialize : (solver == CUMF_SOLVER_LU ? kModeLU : kModeCG);
  info[0] = facts.n_dual;
  info[1] = n_dual6;
  info[2] = facts.n_empty;
  info[3] = route_for(f, mode, facts, switches()).n_dual;
  return 0;
}
