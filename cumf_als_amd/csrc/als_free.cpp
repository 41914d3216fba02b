// als_free.cpp -- host side of the matrix-free CG: a plan's segment lists and the driver of a half-iteration, which the
// implicit route (als_implicit.cpp) uses too, and the explicit entry points of include/cumf_free_capi.h.  Kernels: als_free.hip.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "als_free.h"
#include "cumf_free_capi.h"

using namespace cumf;

void cumf::free_seg_lists(FreeSegLists* l) {
  if (!l) return;
  if (l->d_block) (void)hipFree(l->d_block);
  delete l;
}

// The segments of the plan's rows: a row of n entries starts where its first item does (a cut row's chunks are
// consecutive) and is cut at the offsets 0, kFreeSeg, 2 kFreeSeg, ... from there, whatever the plan's own chunks.
int cumf::plan_free_lists(cumf_plan* p, const FreeSegLists** out) {
  if (!p->free_seg) p->free_seg = new FreeSegLists();
  FreeSegLists* l = p->free_seg;
  *out = l;
  if (l->built) return 0;
  if (l->d_block) {  // an earlier attempt failed half way
    (void)hipFree(l->d_block);
    l->d_block = nullptr;
  }
  const size_t ni = (size_t)p->n_items, rows = (size_t)(p->row_end - p->row_begin);
  std::vector<int> row(ni), rowlen(ni);
  std::vector<long long> begin(ni);
  if (ni) {
    CUMF_HIP_CHECK(hipMemcpy(row.data(), p->d_item_row, ni * sizeof(int), hipMemcpyDeviceToHost));
    CUMF_HIP_CHECK(hipMemcpy(rowlen.data(), p->d_item_rowlen, ni * sizeof(int), hipMemcpyDeviceToHost));
    CUMF_HIP_CHECK(hipMemcpy(begin.data(), p->d_item_begin, ni * sizeof(long long), hipMemcpyDeviceToHost));
  }
  std::vector<long long> start(rows, -1);
  std::vector<int> len(rows, 0);
  for (size_t i = 0; i < ni; ++i) {
    const size_t u = (size_t)(row[i] - p->row_begin);
    if (start[u] < 0 || begin[i] < start[u]) start[u] = begin[i];
    len[u] = rowlen[i];
  }
  std::vector<long long> seg_begin;
  std::vector<int> seg_row, seg_len, row_seg0(rows), row_nseg(rows);
  for (size_t u = 0; u < rows; ++u) {
    row_seg0[u] = (int)seg_row.size();
    for (int o = 0; o < len[u]; o += kFreeSeg) {
      seg_begin.push_back(start[u] + o);
      seg_row.push_back((int)u);
      seg_len.push_back(len[u] - o < kFreeSeg ? len[u] - o : kFreeSeg);
    }
    row_nseg[u] = (int)seg_row.size() - row_seg0[u];
  }
  const size_t ns = seg_row.size();
  std::vector<int> ints;
  for (auto* v : {&seg_row, &seg_len, &row_seg0, &row_nseg, &len}) ints.insert(ints.end(), v->begin(), v->end());
  const size_t bytes = ns * sizeof(long long) + ints.size() * sizeof(int);
  if (bytes) {
    CUMF_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&l->d_block), bytes));
    if (ns) CUMF_HIP_CHECK(hipMemcpy(l->d_block, seg_begin.data(), ns * sizeof(long long), hipMemcpyHostToDevice));
    CUMF_HIP_CHECK(hipMemcpy(l->d_block + ns * sizeof(long long), ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice));
    l->d_seg_begin = reinterpret_cast<long long*>(l->d_block);
    int* d = reinterpret_cast<int*>(l->d_block + ns * sizeof(long long));
    l->d_seg_row = d;
    l->d_seg_len = d + ns;
    l->d_row_seg0 = d + 2 * ns;
    l->d_row_nseg = l->d_row_seg0 + rows;
    l->d_row_len = l->d_row_nseg + rows;
  }
  l->n_seg = (long)ns;
  l->built = true;
  return 0;
}

int cumf::run_matfree(cumf_plan* p, FreeArgs* a, const int* colidx, const float* val, const float* gather, float* update,
                      float lambda, int cg_iters, int kind_vec, int kind_part, int kind_words, hipStream_t s,
                      const std::function<hipError_t(int step, int steps)>& launch) {
  const FreeSegLists* l = nullptr;
  int rc = plan_free_lists(p, &l);
  if (rc) return rc;
  const long rows = p->row_end - p->row_begin;
  if (rows <= 0) return 0;
  const int f = p->f;
  a->seg_row = l->d_seg_row;
  a->seg_begin = l->d_seg_begin;
  a->seg_len = l->d_seg_len;
  a->row_seg0 = l->d_row_seg0;
  a->row_nseg = l->d_row_nseg;
  a->row_len = l->d_row_len;
  a->rows = rows;
  a->nseg = l->n_seg;
  a->colidx = colidx;
  a->val = val;
  a->gather = gather;
  a->x = update + (size_t)p->row_begin * f;
  a->f = f;
  a->lambda = lambda;
  float *vec = nullptr, *part = nullptr, *words = nullptr;
  if ((rc = scratch(s, kind_vec, 2 * (size_t)rows * f, &vec)) || (rc = scratch(s, kind_part, 2 * (size_t)a->nseg * f, &part)) ||
      (rc = scratch(s, kind_words, 2 * (size_t)rows, &words)))
    return rc;
  a->r = vec;
  a->p = vec + (size_t)rows * f;
  a->part = part;
  a->bpart = part + (size_t)a->nseg * f;
  a->rs = words;
  a->done = reinterpret_cast<int*>(words + rows);
  CUMF_HIP_CHECK(hipMemsetAsync(a->done, 0, (size_t)rows * sizeof(int), s));
  const int steps = cg_iters > 0 ? cg_iters : 0;
  for (int k = 0; k <= steps; ++k) CUMF_HIP_CHECK(launch(k, steps));
  return 0;
}

extern "C" int cumf_matfree_available(int f) { return matfree_f_ok(f); }

extern "C" int cumf_als_update_matfree(cumf_plan_t* p, const int* colidx, const float* val, const float* gather, float* update,
                                       float lambda, int cg_iters, void* stream) {
  if (!p || !colidx || !val || !gather || !update) {
    fprintf(stderr, "cumf_als_update_matfree: plan, colidx, val, gather and update must not be NULL\n");
    return (int)hipErrorInvalidValue;
  }
  if (!matfree_f_ok(p->f)) {
    fprintf(stderr, "cumf_als_update_matfree: needs a plan of even 8 <= f <= 512 (got %d)\n", p->f);
    return (int)hipErrorInvalidValue;
  }
  const hipStream_t s = static_cast<hipStream_t>(stream);
  ScratchLease lease;
  FreeArgs a{};
  return run_matfree(p, &a, colidx, val, gather, update, lambda, cg_iters, kScratchFreeVec, kScratchFreePart, kScratchFreeWords, s,
                     [&](int step, int steps) { return launch_free_pass(a, step, steps, s); });
}
