// als_rank.h -- full ranking, held-out ranks and their metrics: what als_rank.hip (kernels) and als_rank.cpp (host side;
// include/cumf_rank_capi.h) share.
#ifndef CUMF_ALS_RANK_H_
#define CUMF_ALS_RANK_H_

#include "als_internal.h"
#include "als_topk.h"

namespace cumf {

constexpr int kRankPoolW = 768;            // held-out keys (and buckets) a wave keeps in LDS for its kTopkQW queries
constexpr int kRankPool = 4 * kRankPoolW;  // ... per workgroup; a wave whose queries have more works on the global arrays
constexpr int kRankMaxK = 16;              // cut-offs per cumf_rank_metrics call
constexpr int kRankCols = 7;               // per-query metric columns in front of the 3 per cut-off
struct RankArgs : ScoreArgs {
  const void* test_rowptr;  // rows + 1 entries, int32 or int64 (test_rowptr64)
  int test_rowptr64;
  const int* test_colidx;
  long long n_test;         // entries of test_colidx (and of keys, hist, ranks)
  unsigned long long* keys; // per held-out entry: its key (0: not eligible), sorted in descending order within each row
  int* hist;                // per row: bucket b = eligible candidates below exactly b of the row's valid keys
  int* nvalid;              // per query: its non-zero keys
  int* ranks;
  int* n_eligible;
};
struct RankKs {
  int n;
  int k[kRankMaxK];
};
int rank_count_occupancy(bool multi);  // workgroups per CU of the count kernel
// keys + ranks = -1 of the entries that are not eligible, the sort of each row, nvalid; hist and n_eligible zeroed
hipError_t launch_rank_thresholds(const RankArgs& a, hipStream_t stream);
hipError_t launch_rank_count(const RankArgs& a, long long grid, hipStream_t stream);
hipError_t launch_rank_finish(const RankArgs& a, hipStream_t stream);
// keys: n_test; part: (kRankCols + 3 ks.n) x rows doubles; out: 6 + 3 ks.n doubles
hipError_t launch_rank_metrics(const int* ranks, const int* n_eligible, long long rows, const void* rowptr, int rowptr64,
                               const float* val, long long n_test, const RankKs& ks, unsigned long long* keys, double* part,
                               double* out, hipStream_t stream);

}  // namespace cumf

#endif  // CUMF_ALS_RANK_H_
