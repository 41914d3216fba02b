// als_weighted.h -- weighted ALS: what als_weighted.hip (kernels) and als_weighted.cpp (host side; include/cumf_weighted_capi.h)
// share.  The third and fourth clients of the matrix-free core (als_free_core.h) and of its host driver (run_matfree,
// als_free.h).
//
// A stored entry (u, i) has the rating r and the weight w >= 0, every unstored entry the target 0 and the weight w0 >= 0:
//   A_u = w0 G + sum_{i in R(u)} (w - w0) y_i y_i^T + reg_u I,  G = Y^T Y,  b_u = sum_{i in R(u)} w r y_i,
// reg_u = (float)n_u lambda or lambda (the reg modes of als_implicit.h).  The kernels only ever evaluate
//   A_u v = w0 (G v) + T_u^T ((w - w0) o (T_u v)) + reg_u v.
// Rank-one weights on the unstored entries (the fourth client): unstored (u, i) weighs a_u c_i, a = own_w0 over the rows being
// updated, c = gather_w0 over the rows of `gather`:
//   A_u = a_u G_c + sum_{i in R(u)} (w - a_u c_i) y_i y_i^T + reg_u I,  G_c = Y^T diag(c) Y (launch_weighted_gram),
//   A_u v = a_u (G_c v) + T_u^T ((w - a_u c) o (T_u v)) + reg_u v.
#ifndef CUMF_ALS_WEIGHTED_H_
#define CUMF_ALS_WEIGHTED_H_

#include "als_implicit.h"  // ImplicitFreeArgs, which WeightedFreeArgs extends; the fp64 Gram and kImpLossBlocks of the loss

namespace cumf {

struct WeightedFreeArgs : ImplicitFreeArgs {  // (alpha is not read)
  const float* wgt;  // the weight of each stored entry, indexed as val
  float w0;          // the weight of every unstored entry; 0: G is not read and may be null
};
// the passes of launch_free_pass, on the weighted kernels
hipError_t launch_weighted_free_pass(const WeightedFreeArgs& a, int step, int cg_iters, hipStream_t stream);
struct WeightedRank1Args : WeightedFreeArgs {  // (w0 is not read; G is the Gram of `gather` weighted by gather_w0)
  const float* own_w0;     // rows: indexed as x, done and row_len (own_w0 of the whole side + row_begin)
  const float* gather_w0;  // indexed as the rows of `gather`
};
// ... on the rank-one kernels
hipError_t launch_weighted_rank1_pass(const WeightedRank1Args& a, int step, int cg_iters, hipStream_t stream);
// The objective from the stored entries and the two fp64 Grams Gx = X^T X, Gy = Y^T Y; part: kImpLossBlocks doubles
hipError_t launch_weighted_loss(const int* rowptr, const int* colidx, const float* val, const float* wgt, const float* XT,
                                const float* thetaT, long m, int f, float lambda, float w0, int reg_mode, const double* Gx,
                                const double* Gy, double* part, double* out, hipStream_t stream);
// The rank-one objective from the stored entries and the two weighted fp64 Grams Gx = X^T diag(row_w0) X, Gy = Y^T diag(col_w0)
// Y; part: 2 kImpLossBlocks doubles
hipError_t launch_weighted_rank1_loss(const int* rowptr, const int* colidx, const float* val, const float* wgt, const float* XT,
                                      const float* thetaT, const float* row_w0, const float* col_w0, long m, long n, int f,
                                      float lambda, int reg_mode, const double* Gx, const double* Gy, double* part, double* out,
                                      hipStream_t stream);

}  // namespace cumf

#endif  // CUMF_ALS_WEIGHTED_H_
