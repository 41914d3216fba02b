// als_free.h -- the matrix-free CG, which trains without ever forming a row's system: what its two routes share.  The explicit
// route is als_free.hip (kernels) and als_free.cpp (host side; include/cumf_free_capi.h); the implicit route
// (als_implicit_free.hip, als_implicit.cpp) extends the arguments here by G and the confidence weights (als_implicit.h).
// The device core of both is als_free_core.h.
//
// Explicit: for a row u with n = n_u > 0 stored entries, T_u the n x f block of gathered factor rows and r_u its ratings:
//   A_u = T_u^T T_u + reg I,  reg = (float)n * lambda in fp32 (oracle/als_oracle_impl.h),  b_u = T_u^T r_u,
// solved by the project's CG (warm start from `update`, at most cg_iters steps, a row ends when r.r < 1e-4 after a step and
// is frozen bit for bit from then on).  The kernels only ever evaluate A_u v = T_u^T (T_u v) + reg v.
// Rows WITHOUT stored entries get x = 0, as the implicit and biased routes give them; the oracle's CG on the all-zero system
// such a row has would divide 0 by 0 and return NaN.
#ifndef CUMF_ALS_FREE_H_
#define CUMF_ALS_FREE_H_

#include <functional>

#include "als_internal.h"

namespace cumf {

// the f both routes take (and the wide Gram and the objective the implicit one needs)
inline bool matfree_f_ok(int f) { return f >= 8 && f <= 512 && (f % 2) == 0; }

// Rows are the plan's, indexed by row - row_begin; a row's stored entries are cut into segments of at most kFreeSeg entries
// at fixed offsets from its start.
constexpr int kFreeSeg = 2048;
constexpr int kFreeRows = 32;  // rows per workgroup of a row pass that adds G v (als_free_core.h: free_gram_rows)
constexpr int kFreeRegPlain = 1;  // ... and its reg mode with reg_u = lambda (CUMF_IMPLICIT_REG_PLAIN); else (float)n_u lambda
// The segment lists of a plan (device arrays), built once per plan at the first use by either route (cumf_plan::free_seg) and
// freed with the plan (free_seg_lists, als_internal.h).
struct FreeSegLists {
  bool built = false;
  long n_seg = 0;
  char* d_block = nullptr;           // the device block the arrays below point into
  long long* d_seg_begin = nullptr;  // n_seg: first entry of each segment (index into colidx / val)
  int* d_seg_row = nullptr;          // ... its row
  int* d_seg_len = nullptr;          // ... its entries, at most kFreeSeg
  int* d_row_seg0 = nullptr;         // rows: first segment of each row (its segments are consecutive)
  int* d_row_nseg = nullptr;
  int* d_row_len = nullptr;          // stored entries of the row
};
CUMF_LOCAL int plan_free_lists(cumf_plan* p, const FreeSegLists** out);

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
  float* part;   // nseg x f: T^T (T v) of each segment (implicit: T^T (w o T v))
  float* bpart;  // nseg x f: the segment's part of b (first pass)
  float* rs;     // rows: r.r
  int* done;     // rows: 1 once the row's CG has ended (zeroed before the first pass)
  int f;
  float lambda;
};
// step 0: the sparse pass with v = x (and b), then r = b - A x, p = r; step k >= 1: CG step k with A p.  step == cg_iters: the
// last pass.
hipError_t launch_free_pass(const FreeArgs& a, int step, int cg_iters, hipStream_t stream);

// One matrix-free half-iteration on the plan's rows: fills *a (the FreeArgs part; the caller has set what its route adds) from
// the plan, its segment lists and the call's arrays, takes r | p, the segment partials of A v | b and r.r | done from the
// scratch pool under the caller's three kinds (the caller holds the ScratchLease), zeroes the done flags and runs the
// cg_iters + 1 passes launch(step, steps).
CUMF_LOCAL int run_matfree(cumf_plan* p, FreeArgs* a, const int* colidx, const float* val, const float* gather, float* update,
                           float lambda, int cg_iters, int kind_vec, int kind_part, int kind_words, hipStream_t stream,
                           const std::function<hipError_t(int step, int steps)>& launch);

}  // namespace cumf

#endif  // CUMF_ALS_FREE_H_
