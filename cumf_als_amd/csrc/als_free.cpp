// als_free.cpp -- host side of the matrix-free explicit half-iteration (include/cumf_free_capi.h).  Kernels: als_free.hip; the
// segment lists are the plan's (plan_free_lists of als_implicit.cpp, shared with the implicit matrix-free CG).
#include <hip/hip_runtime.h>

#include <cstdio>

#include "als_free.h"
#include "cumf_free_capi.h"

using namespace cumf;

extern "C" int cumf_matfree_available(int f) { return f >= 8 && f <= 512 && (f % 2) == 0; }

// Done flags zeroed, then cg_iters + 1 passes (FreeArgs); scratch from the pool.
extern "C" int cumf_als_update_matfree(cumf_plan_t* p, const int* colidx, const float* val, const float* gather, float* update,
                                       float lambda, int cg_iters, void* stream) {
  if (!p || !colidx || !val || !gather || !update) {
    fprintf(stderr, "cumf_als_update_matfree: plan, colidx, val, gather and update must not be NULL\n");
    return (int)hipErrorInvalidValue;
  }
  const int f = p->f;
  if (!cumf_matfree_available(f)) {
    fprintf(stderr, "cumf_als_update_matfree: needs a plan of even 8 <= f <= 512 (got %d)\n", f);
    return (int)hipErrorInvalidValue;
  }
  const hipStream_t s = static_cast<hipStream_t>(stream);
  FreeLists l{};
  int rc = plan_free_lists(p, &l);
  if (rc) return rc;
  const long rows = p->row_end - p->row_begin;
  if (rows <= 0) return 0;
  ScratchLease lease;
  FreeArgs a{};
  a.seg_row = l.seg_row;
  a.seg_begin = l.seg_begin;
  a.seg_len = l.seg_len;
  a.row_seg0 = l.row_seg0;
  a.row_nseg = l.row_nseg;
  a.row_len = l.row_len;
  a.rows = rows;
  a.nseg = l.n_seg;
  a.colidx = colidx;
  a.val = val;
  a.gather = gather;
  a.x = update + (size_t)p->row_begin * f;
  a.f = f;
  a.lambda = lambda;
  float *vec = nullptr, *part = nullptr, *words = nullptr;
  if ((rc = scratch(s, kScratchFreeVec, 2 * (size_t)rows * f, &vec)) ||
      (rc = scratch(s, kScratchFreePart, 2 * (size_t)a.nseg * f, &part)) || (rc = scratch(s, kScratchFreeWords, 2 * (size_t)rows, &words)))
    return rc;
  a.r = vec;
  a.p = vec + (size_t)rows * f;
  a.part = part;
  a.bpart = part + (size_t)a.nseg * f;
  a.rs = words;
  a.done = reinterpret_cast<int*>(words + rows);
  CUMF_HIP_CHECK(hipMemsetAsync(a.done, 0, (size_t)rows * sizeof(int), s));
  const int steps = cg_iters > 0 ? cg_iters : 0;
  for (int k = 0; k <= steps; ++k) CUMF_HIP_CHECK(launch_free_pass(a, k, steps, s));
  return 0;
}
