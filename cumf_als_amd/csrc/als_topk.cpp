// als_topk.cpp -- host side of top-k recommendation and ranking metrics (include/cumf_topk_capi.h): argument checks, scratch,
// launches; and score_setup, the set-up every scoring launch shares (als_rank.cpp too): the slab cut (topk_cut, als_topk.h) and
// the common arguments.  Kernels: als_topk.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>

#include "als_topk.h"
#include "cumf_topk_capi.h"

using namespace cumf;

namespace {

bool topk_ok(int f, int k) { return f >= 1 && f <= kTopkMaxF && k >= 1 && k <= kTopkMaxK; }

}  // namespace

int cumf::score_setup(ScoreArgs* a, const float* Q, long long rows, const float* C, long long ncand, int f,
                      const void* excl_rowptr, int rowptr_is_64, const int* excl_colidx, int (*occupancy)(bool multi),
                      long long* grid) {
  *grid = 0;
  if (f < 1 || f > kTopkMaxF || rows < 0 || ncand < 0 || ncand > 0x7fffffffL || (rows > 0 && !Q) || (ncand > 0 && !C) ||
      (!excl_rowptr) != (!excl_colidx))
    return (int)hipErrorInvalidValue;
  if (rows == 0) return 0;
  int dev = 0, cus = 0;
  CUMF_HIP_CHECK(hipGetDevice(&dev));
  CUMF_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const TopkCut cut = topk_cut(rows, ncand, std::max(cus, 1), occupancy(f > kTopkJC));
  a->Q = Q;
  a->rows = rows;
  a->C = C;
  a->ncand = ncand;
  a->f = f;
  a->excl_rowptr = excl_rowptr;
  a->rowptr64 = rowptr_is_64 ? 1 : 0;
  a->excl_colidx = excl_colidx;
  a->vec = (f % 4 == 0) && (reinterpret_cast<uintptr_t>(C) % 16 == 0);
  a->nslab = cut.nslab;
  a->slab_len = cut.slab_len;
  a->n_items = cut.n_items;
  *grid = cut.grid;
  return 0;
}

extern "C" int cumf_topk_available(int f, int k) { return topk_ok(f, k); }

extern "C" int cumf_topk(const float* Q, long rows, const float* C, long ncand, int f, const void* excl_rowptr,
                         int rowptr_is_64, const int* excl_colidx, int k, int* ids, float* scores, void* stream) {
  TopkArgs a{};
  long long grid = 0;
  int rc = (int)hipErrorInvalidValue;
  if (topk_ok(f, k) && (rows <= 0 || (ids && scores)))
    rc = score_setup(&a, Q, rows, C, ncand, f, excl_rowptr, rowptr_is_64, excl_colidx, topk_score_occupancy, &grid);
  if (rc == (int)hipErrorInvalidValue)
    fprintf(stderr,
            "cumf_topk: needs 1 <= f <= %d (got %d), 1 <= k <= %d (got %d), rows >= 0, 0 <= ncand < 2^31, the tables and "
            "outputs, and both exclusion arrays or neither\n",
            kTopkMaxF, f, kTopkMaxK, k);
  if (rc || !grid) return rc;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  ScratchLease lease;
  a.k = k;
  a.ids = ids;
  a.scores = scores;
  rc = scratch(s, kScratchTopkWork, (size_t)grid * kTopkQB * (k + kTopkBuf), &a.work);
  if (!rc && a.nslab > 1) rc = scratch(s, kScratchTopkPart, (size_t)a.nslab * rows * k, &a.part);
  if (rc) return rc;
  CUMF_HIP_CHECK(launch_topk_score(a, grid, s));
  if (a.nslab > 1) CUMF_HIP_CHECK(launch_topk_merge(a.part, rows, k, a.nslab, ids, scores, s));
  return 0;
}

extern "C" int cumf_ranking_metrics(const int* ids, long rows, int k, const void* test_rowptr, int rowptr_is_64,
                                    const int* test_colidx, const float* test_val, double* out4_f64, void* stream) {
  if (k < 1 || rows < 0 || !out4_f64 || (rows > 0 && (!ids || !test_rowptr || !test_colidx))) {
    fprintf(stderr, "cumf_ranking_metrics: needs k >= 1 (got %d), rows >= 0, ids, the held-out CSR and out4_f64\n", k);
    return (int)hipErrorInvalidValue;
  }
  const hipStream_t s = static_cast<hipStream_t>(stream);
  ScratchLease lease;
  double* part = nullptr;
  int rc = scratch(s, kScratchTopkMetrics, (size_t)4 * rows, &part);
  if (rc) return rc;
  CUMF_HIP_CHECK(launch_topk_metrics(ids, rows, k, test_rowptr, rowptr_is_64 ? 1 : 0, test_colidx, test_val, part, out4_f64, s));
  return 0;
}
