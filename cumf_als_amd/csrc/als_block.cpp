// als_block.cpp -- the drivers of a half-iteration of the block solvers (als_block.h), implicit and explicit: the arguments
// from the plan and its segment lists, the explicit solver's row classes, the scratch, and the launches on the caller's
// stream; the explicit entry points of include/cumf_free_capi.h.  Kernels: als_block.hip, als_block_fused.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "als_block.h"
#include "cumf_free_capi.h"
#include "cumf_implicit_capi.h"
#include "cumf_weighted_capi.h"

using namespace cumf;

int cumf::update_block(cumf_plan* p, const int* colidx, const float* val, const float* gather, const float* G, float* update,
                       float lambda, float alpha, int reg_mode, int sweeps, hipStream_t s) {
  const FreeSegLists* l = nullptr;
  int rc = plan_free_lists(p, &l);
  if (rc) return rc;
  const long rows = p->row_end - p->row_begin;
  if (rows <= 0) return 0;
  const int f = p->f, nb = (f + kBlockWidth - 1) / kBlockWidth;
  BlockArgs a{};
  a.seg_row = l->d_seg_row;
  a.seg_begin = l->d_seg_begin;
  a.seg_len = l->d_seg_len;
  a.row_seg0 = l->d_row_seg0;
  a.row_nseg = l->d_row_nseg;
  a.row_len = l->d_row_len;
  a.rows = rows;
  a.nseg = l->n_seg;
  a.ent0 = l->ent_begin;
  a.colidx = colidx;
  a.val = val;
  a.gather = gather;
  a.G = G;
  a.x = update + (size_t)p->row_begin * f;
  a.f = f;
  a.lambda = lambda;
  a.alpha = alpha;
  a.reg_mode = reg_mode;
  // the caller holds the ScratchLease
  if ((rc = scratch(s, kScratchBlockYhat, (size_t)(l->ent_end - l->ent_begin), &a.yhat)) ||
      (rc = scratch(s, kScratchBlockPart, (size_t)a.nseg * kBlockPart, &a.part)) ||
      (rc = scratch(s, kScratchBlockStep, (size_t)rows * kBlockWidth, &a.d)))
    return rc;
  CUMF_HIP_CHECK(launch_block_open(a, s));
  // yhat runs one block step behind x: the step of the very last block is never folded in, nothing reads it
  for (int sweep = 0; sweep < sweeps; ++sweep)
    for (int k = 0; k < nb; ++k) CUMF_HIP_CHECK(launch_block_step(a, k, sweep > 0 || k > 0, sweep == 0, s));
  return 0;
}

void cumf::free_block_rows(BlockRowPlan* b) {
  if (!b) return;
  for (BlockRowLists& l : b->route)
    if (l.d_block) (void)hipFree(l.d_block);
  delete b;
}

// The rows of the plan by how the explicit solver runs them.  A row of at most kBlockCap[c] entries goes to the smallest such
// class c (longest first inside a class: the waves of a workgroup then end together and the long rows start first); a row
// beyond the last class -- under kBlockRouteSegmented every row -- is a long row and keeps its segments of the FreeSegLists.
static int plan_block_rows(cumf_plan* p, const FreeSegLists* fl, int route, const BlockRowLists** out) {
  if (!p->block_rows) p->block_rows = new BlockRowPlan();
  BlockRowLists* l = &p->block_rows->route[route];
  *out = l;
  if (l->built) return 0;
  if (l->d_block) {  // an earlier attempt failed half way
    (void)hipFree(l->d_block);
    l->d_block = nullptr;
  }
  const size_t rows = (size_t)(p->row_end - p->row_begin), ns = (size_t)fl->n_seg;
  std::vector<int> len(rows), seg0(rows), nseg(rows), seg_len(ns);
  std::vector<long long> seg_begin(ns);
  if (rows) {
    CUMF_HIP_CHECK(hipMemcpy(len.data(), fl->d_row_len, rows * sizeof(int), hipMemcpyDeviceToHost));
    CUMF_HIP_CHECK(hipMemcpy(seg0.data(), fl->d_row_seg0, rows * sizeof(int), hipMemcpyDeviceToHost));
    CUMF_HIP_CHECK(hipMemcpy(nseg.data(), fl->d_row_nseg, rows * sizeof(int), hipMemcpyDeviceToHost));
  }
  if (ns) {
    CUMF_HIP_CHECK(hipMemcpy(seg_len.data(), fl->d_seg_len, ns * sizeof(int), hipMemcpyDeviceToHost));
    CUMF_HIP_CHECK(hipMemcpy(seg_begin.data(), fl->d_seg_begin, ns * sizeof(long long), hipMemcpyDeviceToHost));
  }
  std::vector<int> cls[kBlockClasses], lrow, lrow_pseg0, lseg_row, lseg_len;
  std::vector<long long> lseg_begin;
  l->lent_begin = l->lent_end = 0;
  l->lrow_min = 0;
  l->lrow_max = -1;
  for (size_t u = 0; u < rows; ++u) {
    int c = 0;
    while (c < kBlockClasses && len[u] > kBlockCap[c]) ++c;
    if (route == kBlockRouteSegmented) c = kBlockClasses;
    if (c < kBlockClasses) {
      cls[c].push_back((int)u);
      continue;
    }
    if (lrow.empty()) l->lrow_min = (long)u;
    l->lrow_max = (long)u;
    lrow.push_back((int)u);
    lrow_pseg0.push_back((int)lseg_row.size());
    for (int k = 0; k < nseg[u]; ++k) {
      const size_t sg = (size_t)seg0[u] + k;
      if (l->lent_end == 0 || seg_begin[sg] < l->lent_begin) l->lent_begin = seg_begin[sg];
      if (seg_begin[sg] + seg_len[sg] > l->lent_end) l->lent_end = seg_begin[sg] + seg_len[sg];
      lseg_begin.push_back(seg_begin[sg]);
      lseg_row.push_back((int)u);
      lseg_len.push_back(seg_len[sg]);
    }
  }
  for (auto& c : cls) std::stable_sort(c.begin(), c.end(), [&](int x, int y) { return len[x] > len[y]; });
  std::vector<int> ints;
  for (auto* v : {&cls[0], &cls[1], &lrow, &lrow_pseg0, &lseg_row, &lseg_len}) ints.insert(ints.end(), v->begin(), v->end());
  const size_t nl = lseg_begin.size(), bytes = nl * sizeof(long long) + ints.size() * sizeof(int);
  if (bytes) {
    CUMF_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&l->d_block), bytes));
    if (nl) CUMF_HIP_CHECK(hipMemcpy(l->d_block, lseg_begin.data(), nl * sizeof(long long), hipMemcpyHostToDevice));
    if (!ints.empty())
      CUMF_HIP_CHECK(hipMemcpy(l->d_block + nl * sizeof(long long), ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice));
    l->d_lseg_begin = reinterpret_cast<long long*>(l->d_block);
    int* d = reinterpret_cast<int*>(l->d_block + nl * sizeof(long long));
    for (int c = 0; c < kBlockClasses; ++c) {
      l->d_class_rows[c] = d;
      d += cls[c].size();
    }
    l->d_lrow = d;
    l->d_lrow_pseg0 = d + lrow.size();
    l->d_lseg_row = d + 2 * lrow.size();
    l->d_lseg_len = l->d_lseg_row + nl;
  }
  for (int c = 0; c < kBlockClasses; ++c) l->n_class[c] = (long)cls[c].size();
  l->n_lrow = (long)lrow.size();
  l->n_lseg = (long)nl;
  l->built = true;
  return 0;
}

int cumf::update_block_explicit(cumf_plan* p, const int* colidx, const float* val, const float* gather, float* update,
                                float lambda, int sweeps, int route, bool nonneg, long long* stats, hipStream_t s) {
  static_assert(kBlockClasses == 2, "plan_block_rows packs two class lists");
  const FreeSegLists* fl = nullptr;
  int rc = plan_free_lists(p, &fl);
  if (rc) return rc;
  const long rows = p->row_end - p->row_begin;
  if (rows <= 0) return 0;
  const BlockRowLists* l = nullptr;
  if ((rc = plan_block_rows(p, fl, route, &l))) return rc;
  const int f = p->f, nb = (f + kBlockWidth - 1) / kBlockWidth;
  BlockArgs a{};
  a.seg_row = fl->d_seg_row;
  a.seg_begin = fl->d_seg_begin;
  a.seg_len = fl->d_seg_len;
  a.row_seg0 = fl->d_row_seg0;
  a.row_nseg = fl->d_row_nseg;
  a.row_len = fl->d_row_len;
  a.rows = rows;
  a.nseg = fl->n_seg;
  a.ent0 = fl->ent_begin;
  a.colidx = colidx;
  a.val = val;
  a.gather = gather;
  a.x = update + (size_t)p->row_begin * f;
  a.f = f;
  a.lambda = lambda;
  if (l->n_lrow > 0) {
    // the long rows first (they are the longest work): the segment kernels on the compact lists, with yhat over the long rows'
    // span of entries, a partial per long segment and d over the long rows' span of rows
    BlockArgs b = a;
    b.seg_row = l->d_lseg_row;
    b.seg_begin = l->d_lseg_begin;
    b.seg_len = l->d_lseg_len;
    b.nseg = l->n_lseg;
    b.ent0 = l->lent_begin;
    float* d = nullptr;
    if ((rc = scratch(s, kScratchBlockYhat, (size_t)(l->lent_end - l->lent_begin), &b.yhat)) ||
        (rc = scratch(s, kScratchBlockPart, (size_t)b.nseg * kBlockPart, &b.part)) ||
        (rc = scratch(s, kScratchBlockStep, (size_t)(l->lrow_max - l->lrow_min + 1) * kBlockWidth, &d)))
      return rc;
    b.d = d - (size_t)l->lrow_min * kBlockWidth;  // indexed by row
    CUMF_HIP_CHECK(launch_block_open(b, s));
    for (int sweep = 0; sweep < sweeps; ++sweep)
      for (int k = 0; k < nb; ++k)
        CUMF_HIP_CHECK(launch_block_step_explicit(b, l->d_lrow, l->d_lrow_pseg0, l->n_lrow, k, sweep > 0 || k > 0, sweep == 0, nonneg,
                                                 stats, s));
  }
  for (int c = kBlockClasses - 1; c >= 0; --c)
    CUMF_HIP_CHECK(launch_block_fused(a, l->d_class_rows[c], l->n_class[c], kBlockCap[c], sweeps, nonneg, stats, s));
  return 0;
}

// The weighted half-iteration: update_block_explicit's routing on the weighted kernels.  Without a Gram term (w0 == 0 and no
// rank-one vectors) the fused kernel is block_fused_kernel at kFreeWeightArray and the long rows end in block_row_free_kernel;
// with one, block_fused_gram_kernel and the scaled block_row_kernel over the long rows' list.  nonneg: the same launches at
// kNonneg; stats as update_block_explicit takes them.
int cumf::update_block_weighted(cumf_plan* p, const int* colidx, const float* val, const float* wgt, const float* gather,
                                const float* G, const float* own_w0, const float* gather_w0, float* update, float lambda,
                                float w0, int reg_mode, int sweeps, int route, bool nonneg, long long* stats, hipStream_t s) {
  const FreeSegLists* fl = nullptr;
  int rc = plan_free_lists(p, &fl);
  if (rc) return rc;
  const long rows = p->row_end - p->row_begin;
  if (rows <= 0) return 0;
  const BlockRowLists* l = nullptr;
  if ((rc = plan_block_rows(p, fl, route, &l))) return rc;
  const int f = p->f, nb = (f + kBlockWidth - 1) / kBlockWidth;
  const int mode = own_w0 ? kBlockWeightRank1 : w0 > 0.f ? kBlockWeightScalar : kBlockWeightPlain;
  BlockArgs a{};
  a.seg_row = fl->d_seg_row;
  a.seg_begin = fl->d_seg_begin;
  a.seg_len = fl->d_seg_len;
  a.row_seg0 = fl->d_row_seg0;
  a.row_nseg = fl->d_row_nseg;
  a.row_len = fl->d_row_len;
  a.rows = rows;
  a.nseg = fl->n_seg;
  a.ent0 = fl->ent_begin;
  a.colidx = colidx;
  a.val = val;
  a.gather = gather;
  a.G = G;
  a.x = update + (size_t)p->row_begin * f;
  a.f = f;
  a.lambda = lambda;
  a.reg_mode = reg_mode;
  a.wgt = wgt;
  a.own_w0 = own_w0 ? own_w0 + p->row_begin : nullptr;  // the kernels index rows from the plan's first, as they do x
  a.gather_w0 = gather_w0;
  a.w0 = w0;
  if (l->n_lrow > 0) {  // the long rows first, as update_block_explicit runs them
    BlockArgs b = a;
    b.seg_row = l->d_lseg_row;
    b.seg_begin = l->d_lseg_begin;
    b.seg_len = l->d_lseg_len;
    b.nseg = l->n_lseg;
    b.ent0 = l->lent_begin;
    float* d = nullptr;
    if ((rc = scratch(s, kScratchBlockYhat, (size_t)(l->lent_end - l->lent_begin), &b.yhat)) ||
        (rc = scratch(s, kScratchBlockPart, (size_t)b.nseg * kBlockPart, &b.part)) ||
        (rc = scratch(s, kScratchBlockStep, (size_t)(l->lrow_max - l->lrow_min + 1) * kBlockWidth, &d)))
      return rc;
    b.d = d - (size_t)l->lrow_min * kBlockWidth;  // indexed by row
    CUMF_HIP_CHECK(launch_block_open(b, s));
    for (int sweep = 0; sweep < sweeps; ++sweep)
      for (int k = 0; k < nb; ++k)
        CUMF_HIP_CHECK(launch_block_step_weighted(b, l->d_lrow, l->d_lrow_pseg0, l->n_lrow, k, sweep > 0 || k > 0, sweep == 0, mode,
                                                 nonneg, stats, s));
  }
  for (int c = kBlockClasses - 1; c >= 0; --c)
    if (mode == kBlockWeightPlain)
      CUMF_HIP_CHECK(launch_block_fused_weighted(a, l->d_class_rows[c], l->n_class[c], kBlockCap[c], sweeps, nonneg, stats, s));
    else
      CUMF_HIP_CHECK(launch_block_fused_gram(a, l->d_class_rows[c], l->n_class[c], kBlockCap[c], sweeps, mode, nonneg, stats, s));
  return 0;
}

// the two weighted entry points: one set of refusals
static int weighted_block_entry(const char* who, const cumf_plan_t* pc, const int* colidx, const float* val, const float* wgt,
                                const float* gather, const float* G, const float* own_w0, const float* gather_w0, float* update,
                                float lambda, float w0, int reg_mode, int sweeps, int route, bool nonneg, long long* stats,
                                void* stream) {
  if (!pc || !colidx || !val || !wgt || !gather || !update) {
    fprintf(stderr, "%s: plan, colidx, val, wgt, gather and update must not be NULL\n", who);
    return (int)hipErrorInvalidValue;
  }
  if (!block_f_ok(pc->f)) {
    fprintf(stderr, "%s: needs a plan of even 8 <= f <= 512 (got %d)\n", who, pc->f);
    return (int)hipErrorInvalidValue;
  }
  if ((reg_mode != CUMF_IMPLICIT_REG_WEIGHTED && reg_mode != CUMF_IMPLICIT_REG_PLAIN) || !(w0 >= 0.f) || sweeps < 1) {
    fprintf(stderr, "%s: needs reg_mode 0 or 1 (got %d), w0 >= 0 (got %g) and sweeps >= 1 (got %d)\n", who, reg_mode, (double)w0,
            sweeps);
    return (int)hipErrorInvalidValue;
  }
  if (route != CUMF_BLOCK_ROUTE_AUTO && route != CUMF_BLOCK_ROUTE_SEGMENTED) {
    fprintf(stderr, "%s: unknown route %d (CUMF_BLOCK_ROUTE_AUTO | CUMF_BLOCK_ROUTE_SEGMENTED)\n", who, route);
    return (int)hipErrorInvalidValue;
  }
  if (!own_w0 != !gather_w0 || (own_w0 && w0 != 0.f)) {
    fprintf(stderr, "%s: own_w0 and gather_w0 come together, and with them w0 must be 0 (got %g)\n", who, (double)w0);
    return (int)hipErrorInvalidValue;
  }
  if ((own_w0 || w0 > 0.f) && !G) {
    fprintf(stderr, "%s: G must not be NULL when w0 > 0 or the rank-one vectors are given\n", who);
    return (int)hipErrorInvalidValue;
  }
  ScratchLease lease;
  return update_block_weighted(const_cast<cumf_plan*>(pc), colidx, val, wgt, gather, G, own_w0, gather_w0, update, lambda, w0,
                               reg_mode, sweeps, route, nonneg, stats, static_cast<hipStream_t>(stream));
}

extern "C" int cumf_als_update_weighted_block(const cumf_plan_t* pc, const int* colidx, const float* val, const float* wgt,
                                              const float* gather, const float* G, const float* own_w0, const float* gather_w0,
                                              float* update, float lambda, float w0, int reg_mode, int sweeps, int route,
                                              void* stream) {
  return weighted_block_entry("cumf_als_update_weighted_block", pc, colidx, val, wgt, gather, G, own_w0, gather_w0, update, lambda,
                              w0, reg_mode, sweeps, route, false, nullptr, stream);
}

extern "C" int cumf_als_update_weighted_block_nonneg(const cumf_plan_t* pc, const int* colidx, const float* val, const float* wgt,
                                                     const float* gather, const float* G, const float* own_w0,
                                                     const float* gather_w0, float* update, float lambda, float w0, int reg_mode,
                                                     int sweeps, int route, long long* stats, void* stream) {
  return weighted_block_entry("cumf_als_update_weighted_block_nonneg", pc, colidx, val, wgt, gather, G, own_w0, gather_w0, update,
                              lambda, w0, reg_mode, sweeps, route, true, stats, stream);
}

extern "C" int cumf_block_available(int f) { return block_f_ok(f); }

// the two explicit entry points: one set of refusals
static int block_entry(const char* who, cumf_plan_t* p, const int* colidx, const float* val, const float* gather, float* update,
                       float lambda, int sweeps, int route, bool nonneg, long long* stats, void* stream) {
  if (!p || !colidx || !val || !gather || !update) {
    fprintf(stderr, "%s: plan, colidx, val, gather and update must not be NULL\n", who);
    return (int)hipErrorInvalidValue;
  }
  if (!block_f_ok(p->f)) {
    fprintf(stderr, "%s: needs a plan of even 8 <= f <= 512 (got %d)\n", who, p->f);
    return (int)hipErrorInvalidValue;
  }
  if (sweeps < 1) {
    fprintf(stderr, "%s: needs sweeps >= 1 (got %d)\n", who, sweeps);
    return (int)hipErrorInvalidValue;
  }
  if (route != CUMF_BLOCK_ROUTE_AUTO && route != CUMF_BLOCK_ROUTE_SEGMENTED) {
    fprintf(stderr, "%s: unknown route %d (CUMF_BLOCK_ROUTE_AUTO | CUMF_BLOCK_ROUTE_SEGMENTED)\n", who, route);
    return (int)hipErrorInvalidValue;
  }
  ScratchLease lease;
  return update_block_explicit(p, colidx, val, gather, update, lambda, sweeps, route, nonneg, stats,
                               static_cast<hipStream_t>(stream));
}

extern "C" int cumf_als_update_block(cumf_plan_t* p, const int* colidx, const float* val, const float* gather, float* update,
                                     float lambda, int sweeps, int route, void* stream) {
  return block_entry("cumf_als_update_block", p, colidx, val, gather, update, lambda, sweeps, route, false, nullptr, stream);
}

extern "C" int cumf_als_update_block_nonneg(cumf_plan_t* p, const int* colidx, const float* val, const float* gather,
                                            float* update, float lambda, int sweeps, int route, long long* stats, void* stream) {
  return block_entry("cumf_als_update_block_nonneg", p, colidx, val, gather, update, lambda, sweeps, route, true, stats, stream);
}
