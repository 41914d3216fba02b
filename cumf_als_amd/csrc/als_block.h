// als_block.h -- the block Gauss-Seidel solvers: the iALS++ block solver of implicit feedback (CUMF_SOLVER_BLOCK,
// include/cumf_implicit_capi.h), the explicit block solver (cumf_als_update_block, include/cumf_free_capi.h) and the weighted
// one (cumf_als_update_weighted_block, include/cumf_weighted_capi.h): what als_block.hip, als_block_fused.hip and
// als_block_gram.hip (kernels; device core als_block_core.h) and als_block.cpp (the drivers of a half-iteration) share.
//
// Exact block Gauss-Seidel on each row's normal equations A x = b (A = G + sum_e w_e t_e t_e^T + reg I, t_e the gathered factor
// row of stored entry e).  Blocks are B = kBlockWidth consecutive features, pi_k = [B k, min(B k + B, f)).  With a cached
// prediction yhat_e = t_e . x per stored entry, one block step is
//   g   = sum_e t_e[pi_k] ((1 + w_e) p_e - w_e yhat_e)
//   H   = sum_e w_e t_e[pi_k] t_e[pi_k]^T + G[pi_k, pi_k] + reg I
//   rhs = g - (G x)[pi_k] - reg x[pi_k]
//   d   = H^-1 rhs;  x[pi_k] += d;  yhat_e += t_e[pi_k] . d     (the last folded into the next step's sparse pass)
// and touches only the block's B-float slice of each gathered row.  Every live row runs exactly `sweeps` sweeps over all
// blocks; every sum runs in a fixed order (no float atomics), so a row's result depends on neither its neighbours nor the plan.
//
// Explicit feedback (als_free.h's conventions) is the same recurrence with w = 1, c_e = r_e - yhat_e and no G:
// A = T^T T + reg I, reg = (float)n lambda, rhs = g - reg x[pi_k].  A row of at most kFreeSeg entries runs its whole
// half-iteration on one wave in one launch (block_fused_kernel); longer rows run on the segment kernels, and both routes give
// a row the same bits.
//
// The non-negative explicit solver (cumf_als_update_block_nonneg) changes the block step alone: with c = rhs + H x[pi_k],
//   z = argmin_{z >= 0} 1/2 z^T H z - c^T z;   d = z - x[pi_k];   x[pi_k] = z
// -- block coordinate descent on the row's strictly convex QP, which converges to the row's NNLS solution and is that solution
// after one sweep at f <= 32.  Same kernels (template flag kNonneg), lists, classes and scratch.  The weighted solver
// (cumf_als_update_weighted_block_nonneg) takes the same step on its own H and rhs below, Gram term included: (G x)[pi_k] is
// kept current with d = z - x[pi_k] exactly as with the unconstrained d.
#ifndef CUMF_ALS_BLOCK_H_
#define CUMF_ALS_BLOCK_H_

#include "als_free.h"  // the segment lists the kernels run on

namespace cumf {

constexpr int kBlockWidth = 32;
// one partial per segment and block step: the tiles H00 | H01 | H11 (16 x 16, row-major) and g
constexpr int kBlockPart = 3 * 256 + kBlockWidth;

inline bool block_f_ok(int f) { return matfree_f_ok(f); }

struct BlockArgs {
  const int* seg_row;          // the plan's FreeSegLists (als_free.h)
  const long long* seg_begin;
  const int* seg_len;
  const int* row_seg0;
  const int* row_nseg;
  const int* row_len;
  long long rows, nseg;
  long long ent0;      // first stored entry of the plan's rows: yhat is indexed by entry - ent0
  const int* colidx;
  const float* val;
  const float* gather;
  const float* G;      // f x f Gram of `gather`
  float* x;            // update + row_begin * f: warm start in, solution out
  float* yhat;         // one per stored entry of the plan: t_e . x, one block step behind x
  float* part;         // nseg x kBlockPart
  float* d;            // rows x kBlockWidth: the step of the block solved last
  int f;
  float lambda, alpha;
  int reg_mode;        // kFreeRegPlain: reg = lambda, else (float)n lambda
  // the weighted clients (kFreeWeightArray / kFreeWeightRank1 of als_free_core.h; appended, so the fields above keep their
  // kernel-argument offsets)
  const float* wgt;        // the weight of each stored entry, indexed as val
  const float* own_w0;     // rank-one form: the row's factor of its unstored weights, indexed as the rows of x; else NULL
  const float* gather_w0;  // ... and the column's, indexed as the rows of `gather`
  float w0;                // scalar form: the weight of every unstored entry
};

// yhat_e = t_e . x of every stored entry
hipError_t launch_block_open(const BlockArgs& a, hipStream_t stream);
// block step k: the sparse pass (have_prev: first yhat += t[pi_prev] . d of the step before, prev = k - 1 or the last block)
// and the row pass (first: rows without stored entries are zeroed)
hipError_t launch_block_step(const BlockArgs& a, int k, int have_prev, int first, hipStream_t stream);

// ---- explicit feedback
// Entries a fused row may have, by class: LDS per workgroup of four waves is 4 x (4 224 + 4 cap) B.  The kernel's registers
// allow five waves per SIMD (four at f > 320), that is five workgroups per CU, and cap = 960 is the largest that lets five
// workgroups share the CU's 160 KB (5 x 32 256 B); cap = kFreeSeg leaves three.
constexpr int kBlockClasses = 2;
constexpr int kBlockCap[kBlockClasses] = {960, kFreeSeg};
enum { kBlockRouteAuto = 0, kBlockRouteSegmented = 1 };  // CUMF_BLOCK_ROUTE_* of cumf_free_capi.h

// The rows of a plan as the explicit block solver runs them, per route (device arrays, built on the plan at first use beside
// its FreeSegLists and freed with it): the fused rows of each capacity class, longest first (rows without entries are of the
// first class), and the long rows (kBlockRouteSegmented: every row) with their segments, compact.
struct BlockRowLists {
  bool built = false;
  char* d_block = nullptr;
  long n_class[kBlockClasses] = {};
  int* d_class_rows[kBlockClasses] = {};
  long n_lrow = 0, n_lseg = 0;
  int* d_lrow = nullptr;        // n_lrow: the long rows
  int* d_lrow_pseg0 = nullptr;  // ... the first segment of each in the compact segment list
  long long* d_lseg_begin = nullptr;  // n_lseg: as FreeSegLists, the long rows' segments only
  int* d_lseg_row = nullptr;
  int* d_lseg_len = nullptr;
  long long lent_begin = 0, lent_end = 0;  // the long rows' entries lie in [lent_begin, lent_end)
  long lrow_min = 0, lrow_max = -1;        // ... and the long rows in [lrow_min, lrow_max]
};
struct BlockRowPlan {
  BlockRowLists route[2];
};

// rows[0 .. nrows) of at most `cap` entries each, one wave per row: the whole half-iteration (als_block_fused.hip); a's lists
// are the plan's FreeSegLists
// nonneg: the block step under x >= 0 (block_nnls32, als_block_core.h); stats: NULL or device int64[2], ADDED to: (blocks not
// converged, eliminations)
hipError_t launch_block_fused(const BlockArgs& a, const int* rows, long long nrows, int cap, int sweeps, bool nonneg,
                              long long* stats, hipStream_t stream);
// block step k of the rows `rows` whose segments are a's lists: block_sparse_kernel<32, kFreeWeightNone> and the Gram-free row
// pass block_row_free_kernel (pseg0: first partial of each row)
hipError_t launch_block_step_explicit(const BlockArgs& a, const int* rows, const int* pseg0, long long nrows, int k,
                                      int have_prev, int first, bool nonneg, long long* stats, hipStream_t stream);

// ---- weighted feedback (include/cumf_weighted_capi.h: cumf_als_update_weighted_block).  With s_u the weight of row u's
// unstored entries (w0, or own_w0[u]) and q_e = w_e - s_u c_j the recurrence above runs on
//   A_u = s_u G + sum_e q_e t_e t_e^T + reg I,   b_u = sum_e w_e r_e t_e:
//   g = sum_e t_e[pi_k] (w_e r_e - q_e yhat_e),  H = sum_e q_e t t^T + s_u G[pi_k, pi_k] + reg I,
//   rhs = (g - s_u (G x)[pi_k]) - reg x[pi_k].
// q_e may be negative; H = s_u sum_unstored + sum_stored w + reg I stays positive definite.  BlockWeightMode: where s_u and
// q_e come from; kBlockWeightPlain is the call without any Gram term (w0 == 0, no rank-one vectors: q_e = w_e).
enum BlockWeightMode { kBlockWeightPlain = 0, kBlockWeightScalar = 1, kBlockWeightRank1 = 2 };
// rows[0 .. nrows) of at most `cap` entries, one wave per row, kBlockWeightPlain: block_fused_kernel at kFreeWeightArray.
// nonneg, stats: as launch_block_fused takes them, here and in the two launches below
hipError_t launch_block_fused_weighted(const BlockArgs& a, const int* rows, long long nrows, int cap, int sweeps, bool nonneg,
                                       long long* stats, hipStream_t stream);
// ... with the Gram term (als_block_gram.hip: block_fused_gram_kernel); a.G is required
hipError_t launch_block_fused_gram(const BlockArgs& a, const int* rows, long long nrows, int cap, int sweeps, int mode,
                                   bool nonneg, long long* stats, hipStream_t stream);
// block step k of the rows `rows` on a's segment lists: block_sparse_kernel at the mode's weights, then block_row_free_kernel
// (kBlockWeightPlain) or the Gram row pass block_row_kernel with the row's scale, 32 listed rows per workgroup
hipError_t launch_block_step_weighted(const BlockArgs& a, const int* rows, const int* pseg0, long long nrows, int k,
                                      int have_prev, int first, int mode, bool nonneg, long long* stats, hipStream_t stream);
// One weighted block-solver half-iteration on the plan's rows (als_block.cpp), routed as update_block_explicit routes.
CUMF_LOCAL int update_block_weighted(cumf_plan* p, const int* colidx, const float* val, const float* wgt, const float* gather,
                                     const float* G, const float* own_w0, const float* gather_w0, float* update, float lambda,
                                     float w0, int reg_mode, int sweeps, int route, bool nonneg, long long* stats,
                                     hipStream_t stream);
// One explicit block-solver half-iteration on the plan's rows (als_block.cpp): at most kBlockClasses fused launches, and
// 1 + 2 sweeps ceil(f / B) launches over the long rows where the plan has any.  The caller holds the ScratchLease.
CUMF_LOCAL int update_block_explicit(cumf_plan* p, const int* colidx, const float* val, const float* gather, float* update,
                                     float lambda, int sweeps, int route, bool nonneg, long long* stats, hipStream_t stream);

// One block-solver half-iteration on the plan's rows (als_block.cpp): 1 + 2 sweeps ceil(f / B) launches on `stream`.
CUMF_LOCAL int update_block(cumf_plan* p, const int* colidx, const float* val, const float* gather, const float* G,
                            float* update, float lambda, float alpha, int reg_mode, int sweeps, hipStream_t stream);

}  // namespace cumf

#endif  // CUMF_ALS_BLOCK_H_
