// als_topk.h -- top-k recommendation and ranking metrics: what als_topk.hip (kernels) and als_topk.cpp (host side;
// include/cumf_topk_capi.h) share.  Full ranking scores the same way and cuts the work the same way: als_rank.h and als_score.h
// build on the constants and on topk_cut here.
#ifndef CUMF_ALS_TOPK_H_
#define CUMF_ALS_TOPK_H_

#include <algorithm>

#include "als_internal.h"

namespace cumf {

constexpr int kTopkThreads = 256;         // four waves
constexpr int kTopkQW = 32;               // queries per wave (two 16-row MFMA tiles)
constexpr int kTopkQB = 4 * kTopkQW;      // queries per workgroup
constexpr int kTopkNC = 64;               // candidates per LDS block (four 16-column tiles; one 64-bit exclusion mask)
constexpr int kTopkJC = 128;              // features per LDS chunk
constexpr int kTopkPitch = kTopkJC + 4;   // LDS row pitch: the 16 rows one k-group reads start 4 banks apart
constexpr int kTopkBuf = 128;             // survivor buffer per query (merged when above kTopkBuf - kTopkNC)
constexpr int kTopkMaxK = 128;
constexpr int kTopkMaxF = 512;
// What the scoring kernels share (als_score.h): the two tables, the exclusion CSR and the cut.  TopkArgs and RankArgs
// (als_rank.h) extend it; score_setup fills it.
struct ScoreArgs {
  const float* Q;
  long long rows;
  const float* C;
  long long ncand;
  int f;
  int rowptr64;
  const void* excl_rowptr;  // rows + 1 entries, int32 or int64 (rowptr64); null: no exclusion
  const int* excl_colidx;
  int vec;                  // C rows may be read as float4 (f % 4 == 0, 16-byte aligned)
  int nslab;
  long long slab_len;       // candidates per slab, a multiple of kTopkNC
  long long n_items;        // query blocks x slabs
};
struct TopkArgs : ScoreArgs {
  int k;
  unsigned long long* work; // per workgroup: kTopkQB x (k + kTopkBuf) keys
  unsigned long long* part; // nslab > 1: nslab x rows x k keys
  int* ids;                 // nslab == 1: the result
  float* scores;
};
int topk_score_occupancy(bool multi);  // workgroups per CU of the score kernel
hipError_t launch_topk_score(const TopkArgs& a, long long grid, hipStream_t stream);
hipError_t launch_topk_merge(const unsigned long long* part, long long rows, int k, int nslab, int* ids, float* scores,
                             hipStream_t stream);
// part: 4 x rows doubles; out: (count, precision, recall, ndcg)
hipError_t launch_topk_metrics(const int* ids, long long rows, int k, const void* rowptr, int rowptr64, const int* colidx,
                               const float* val, double* part, double* out, hipStream_t stream);

// How a scoring kernel cuts the work, decided here only: query blocks of kTopkQB x slabs of the candidates, on a persistent
// grid of at most one workgroup per resident slot.  A query block alone takes all candidates (one slab) when there are at
// least two blocks per slot; fewer blocks (few queries, e.g. the items x users side of Netflix) split the candidates into
// slabs until there are, but no slab below kTopkMinSlab candidates.  The result does not depend on the cut.
constexpr long long kTopkMinSlab = 16 * kTopkNC;  // candidates per slab at least: the per-slab set-up stays a small part
struct TopkCut {
  int nslab;
  long long slab_len;
  long long n_items;
  long long grid;
};
inline TopkCut topk_cut(long long rows, long long ncand, int cus, int wgs_per_cu) {
  const long long qblocks = (rows + kTopkQB - 1) / kTopkQB;
  const long long slots = (long long)cus * wgs_per_cu;
  long long nslab = 1;
  if (qblocks < 2 * slots) nslab = (2 * slots + qblocks - 1) / qblocks;
  nslab = std::min(nslab, std::max(1LL, (ncand + kTopkMinSlab - 1) / kTopkMinSlab));
  long long slab_len = (ncand + nslab - 1) / nslab;
  slab_len = std::max((long long)kTopkNC, (slab_len + kTopkNC - 1) / kTopkNC * kTopkNC);
  nslab = std::max(1LL, (ncand + slab_len - 1) / slab_len);
  const long long items = qblocks * nslab;
  return TopkCut{(int)nslab, slab_len, items, std::min(items, slots)};
}

// The host set-up of a scoring launch, for cumf_topk and cumf_heldout_ranks alike: the argument checks they share
// (hipErrorInvalidValue without a message: the caller's names its own function and limits), then the device's CU count, the
// cut at `occupancy(f > kTopkJC)` workgroups per CU and the fields of *a.  rows == 0: returns 0 with *grid = 0 before any
// device query.
int score_setup(ScoreArgs* a, const float* Q, long long rows, const float* C, long long ncand, int f, const void* excl_rowptr,
                int rowptr_is_64, const int* excl_colidx, int (*occupancy)(bool multi), long long* grid);

}  // namespace cumf

#endif  // CUMF_ALS_TOPK_H_
