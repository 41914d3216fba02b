// als_rank.cpp -- host side of full-ranking evaluation (include/cumf_rank_capi.h): argument checks, the set-up shared with
// top-k (score_setup, als_topk.cpp), scratch, launches.  Kernels: als_rank.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>

#include "als_rank.h"
#include "cumf_rank_capi.h"

using namespace cumf;

namespace {

bool rank_ok(int f) { return f >= 1 && f <= kTopkMaxF; }

}  // namespace

extern "C" int cumf_rank_available(int f) { return rank_ok(f); }

extern "C" int cumf_heldout_ranks(const float* Q, long rows, const float* C, long ncand, int f, const void* excl_rowptr,
                                  int excl_rowptr_is_64, const int* excl_colidx, const void* test_rowptr,
                                  int test_rowptr_is_64, const int* test_colidx, long n_test, int* ranks, int* n_eligible,
                                  void* stream) {
  RankArgs a{};
  long long grid = 0;
  int rc = (int)hipErrorInvalidValue;
  if (n_test >= 0 && (rows <= 0 || (n_eligible && test_rowptr)) && (n_test <= 0 || (test_colidx && ranks)))
    rc = score_setup(&a, Q, rows, C, ncand, f, excl_rowptr, excl_rowptr_is_64, excl_colidx, rank_count_occupancy, &grid);
  if (rc == (int)hipErrorInvalidValue)
    fprintf(stderr,
            "cumf_heldout_ranks: needs 1 <= f <= %d (got %d), rows >= 0, 0 <= ncand < 2^31, n_test >= 0, the tables, the "
            "held-out CSR and the outputs, and both exclusion arrays or neither\n",
            kTopkMaxF, f);
  if (rc || !grid) return rc;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  ScratchLease lease;
  a.test_rowptr = test_rowptr;
  a.test_rowptr64 = test_rowptr_is_64 ? 1 : 0;
  a.test_colidx = test_colidx;
  a.n_test = n_test;
  a.ranks = ranks;
  a.n_eligible = n_eligible;
  rc = scratch(s, kScratchRankKeys, (size_t)n_test, &a.keys);
  if (!rc) rc = scratch(s, kScratchRankHist, (size_t)n_test, &a.hist);
  if (!rc) rc = scratch(s, kScratchRankValid, (size_t)rows, &a.nvalid);
  if (rc) return rc;
  CUMF_HIP_CHECK(launch_rank_thresholds(a, s));
  CUMF_HIP_CHECK(launch_rank_count(a, grid, s));
  if (n_test > 0) CUMF_HIP_CHECK(launch_rank_finish(a, s));
  return 0;
}

extern "C" int cumf_rank_metrics(const int* ranks, const int* n_eligible, long rows, const void* test_rowptr,
                                 int rowptr_is_64, const float* test_val, long n_test, const int* ks, int n_k,
                                 double* out_f64, void* stream) {
  bool ok = rows >= 0 && n_test >= 0 && n_k >= 0 && n_k <= kRankMaxK && out_f64 && (n_k == 0 || ks) &&
            (rows == 0 || (n_eligible && test_rowptr)) && (n_test == 0 || ranks);
  for (int c = 0; ok && c < n_k; ++c) ok = ks[c] >= 1;
  if (!ok) {
    fprintf(stderr,
            "cumf_rank_metrics: needs rows >= 0, n_test >= 0, 0 <= n_k <= %d (got %d) cut-offs >= 1, ranks, n_eligible, the "
            "held-out row pointers and out_f64\n",
            kRankMaxK, n_k);
    return (int)hipErrorInvalidValue;
  }
  const hipStream_t s = static_cast<hipStream_t>(stream);
  RankKs k{};
  k.n = n_k;
  for (int c = 0; c < n_k; ++c) k.k[c] = ks[c];
  ScratchLease lease;
  unsigned long long* keys = nullptr;
  double* part = nullptr;
  int rc = scratch(s, kScratchRankKeys, (size_t)n_test, &keys);
  if (!rc) rc = scratch(s, kScratchRankMetrics, (size_t)(kRankCols + 3 * n_k) * rows, &part);
  if (rc) return rc;
  CUMF_HIP_CHECK(launch_rank_metrics(ranks, n_eligible, rows, test_rowptr, rowptr_is_64 ? 1 : 0, test_val, n_test, k, keys, part,
                                     out_f64, s));
  return 0;
}
