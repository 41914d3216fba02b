// als_block.h -- the iALS++ block solver of implicit feedback (CUMF_SOLVER_BLOCK, include/cumf_implicit_capi.h): what
// als_block.hip (kernels) and als_block.cpp (the driver of a half-iteration) share.
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
};

// yhat_e = t_e . x of every stored entry
hipError_t launch_block_open(const BlockArgs& a, hipStream_t stream);
// block step k: the sparse pass (have_prev: first yhat += t[pi_prev] . d of the step before, prev = k - 1 or the last block)
// and the row pass (first: rows without stored entries are zeroed)
hipError_t launch_block_step(const BlockArgs& a, int k, int have_prev, int first, hipStream_t stream);

// One block-solver half-iteration on the plan's rows (als_block.cpp): 1 + 2 sweeps ceil(f / B) launches on `stream`.
CUMF_LOCAL int update_block(cumf_plan* p, const int* colidx, const float* val, const float* gather, const float* G,
                            float* update, float lambda, float alpha, int reg_mode, int sweeps, hipStream_t stream);

}  // namespace cumf

#endif  // CUMF_ALS_BLOCK_H_
