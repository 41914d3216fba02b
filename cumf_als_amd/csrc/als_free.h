// als_free.h -- explicit feedback up to f = 512 without ever forming a system: what als_free.hip (kernels) and als_free.cpp
// (host side; include/cumf_free_capi.h) share.
//
// For a row u with n = n_u > 0 stored entries, T_u the n x f block of gathered factor rows and r_u its ratings:
//   A_u = T_u^T T_u + reg I,  reg = (float)n * lambda in fp32 (oracle/als_oracle_impl.h),  b_u = T_u^T r_u,
// solved by the project's CG (warm start from `update`, at most cg_iters steps, a row ends when r.r < 1e-4 after a step and
// is frozen bit for bit from then on).  The kernels only ever evaluate A_u v = T_u^T (T_u v) + reg v.
// Rows WITHOUT stored entries get x = 0, as the implicit and biased routes give them; the oracle's CG on the all-zero system
// such a row has would divide 0 by 0 and return NaN.
#ifndef CUMF_ALS_FREE_H_
#define CUMF_ALS_FREE_H_

#include "als_implicit.h"  // kFreeSeg, FreeLists, plan_free_lists: the segments both matrix-free routes cut a plan's rows into

namespace cumf {

struct FreeArgs {
  const int* seg_row;          // nseg: row (row - row_begin) of each segment
  const long long* seg_begin;  // ... its first entry (index into colidx / val)
  const int* seg_len;          // ... its entries, at most kFreeSeg
  const int* row_seg0;         // rows: first segment of each row (its segments are consecutive)
  const int* row_nseg;
  const int* row_len;          // stored entries of the row (0: x = 0)
  long long rows, nseg;
  const int* colidx;
  const float* val;
  const float* gather;
  float* x;      // update + row_begin * f: warm start in, solution out
  float* r;      // rows x f residuals
  float* p;      // rows x f search directions
  float* part;   // nseg x f: T^T (T v) of each segment
  float* bpart;  // nseg x f: the segment's part of b (first pass)
  float* rs;     // rows: r.r
  int* done;     // rows: 1 once the row's CG has ended (zeroed before the first pass)
  int f;
  float lambda;
};
// step 0: the sparse pass with v = x (and b), then r = b - A x, p = r; step k >= 1: CG step k with A p.  step == cg_iters: the
// last pass.
hipError_t launch_free_pass(const FreeArgs& a, int step, int cg_iters, hipStream_t stream);

}  // namespace cumf

#endif  // CUMF_ALS_FREE_H_
