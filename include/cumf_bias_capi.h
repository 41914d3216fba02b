/*
 * cumf_bias_capi.h -- C ABI of biased explicit ALS of libALS.so: the baseline-predictor model
 *   r^(u,i) = mu + b_u + c_i + x_u . theta_i
 * with a global mean mu, a bias b_u per user, a bias c_i per item and f factors per user and item.
 *
 * The model.  With Theta and c fixed, row u's update minimises
 *   sum_i (r_ui - mu - c_i - b_u - x_u . theta_i)^2 + n_u (lambda |x_u|^2 + lambda_bias b_u^2)
 * over the n_u ratings of the row: a ridge problem in the f + 1 unknowns (x_u, b_u).  The item side is the mirror image.
 *
 * The identity the half-iteration rests on.  Let s = sqrt(lambda / lambda_bias) and F = f + 2.  The problem above is the
 * plain ALS update at F,  A = sum_i g_i g_i^T + lambda n_u I_F,  rhs = sum_i r'_ui g_i,  A z = rhs,  with
 *   gather rows  g_i = [theta_i | s | 0],   ratings  r'_ui = (r_ui - mu) - c_i,
 * and then  x_u = z[0 .. f),  b_u = s z[f],  z[f + 1] = 0 exactly: that unknown is decoupled, its row and column of the
 * Gram and its right-hand side are zero.  (Substituting b_u = s z[f] turns lambda_bias b_u^2 into lambda z[f]^2.)  So a
 * biased half-iteration runs on the fused kernels of cumf_als_update_fused, every route of them, with a plan made at F.
 * (Some routes return a term of denormal size, below 1e-41, for z[f + 1] instead of 0; step 4 below overwrites it.)
 *
 * Tables.  XA is m x F and TA is n x F, fp32 row-major.  Between calls they are in SERVING form,
 *   XA[u] = [x_u | b_u | 1],   TA[i] = [theta_i | 1 | c_i],
 * so that the plain dot product of two rows is r^ - mu, and cumf_topk / cumf_heldout_ranks on the two tables rank by the
 * biased prediction.  The bias vectors b (m floats) and c (n floats) are arrays of their own and are the truth; columns f
 * and f + 1 of the tables are derived from them by every call.
 *
 * cumf_bias_update is one half-iteration of the plan's rows as one call; it enqueues, in this order:
 *   1. the residual ratings of the plan's entries into pooled scratch, in fp32 with two roundings and no contraction:
 *        r'[e] = fl(fl(val[e] - mu) - gather_bias[colidx[e]]);
 *   2. the training columns, with s = (float)sqrt((double)lambda / (double)lambda_bias) and (own, other) = (f, f + 1) for
 *      side CUMF_BIAS_SIDE_X, (f + 1, f) for CUMF_BIAS_SIDE_THETA:
 *        gather[:, own] = s, gather[:, other] = 0 for every row of the gather table;
 *        update[u, own] = fl(own_bias[u] / s) (the warm start of the CG), update[u, other] = 0 for the plan's rows;
 *   3. what cumf_als_update_fused (or, with sse_bins, cumf_als_update_fused_sse) runs for this plan, these tables, r' and
 *      lambda: the same kernels on the same route, the same bits;
 *   4. own_bias[u] = fl(update[u, own] * s) for the plan's rows; rows of the plan without ratings get x = 0 and bias 0
 *      (the fused kernels leave NaN there); both tables back in serving form.
 * The plan must have been made at F = f + 2 over the side's row pointer, and its gather-row count set
 * (cumf_plan_set_gather_rows).  Both tables are modified during the call: no other stream may read them meanwhile.  With
 * sse_bins (CUMF_SSE_BINS doubles, added to) the call also delivers the biased model's train SSE of the plan's rows -- the
 * fused SSE of the residual system is exactly that -- under the contract of cumf_als_update_fused_sse, and is available
 * exactly when cumf_fused_sse_available says so for the plan.
 *
 * Prediction.  For a pair (u, i) the score is the fp32 fmaf chain of cumf_topk_capi.h over the augmented rows,
 *   s = +0.0f;  for j = 0 .. F - 1:  s = fmaf(XA[u,j], TA[i,j], s),
 * and cumf_bias_predict writes out[e] = clamp(fl(mu + s_e), lo, hi); lo = -inf and hi = +inf do not clip; a NaN stays NaN.
 * cumf_bias_sse writes the sum over the entries of d^2 with d = fl(val[e] - fl(mu + s_e)), unclipped, squared and summed
 * in fp64.  cumf_bias_mean writes the fp64 mean of val; mu is its rounding to fp32.  Both sums run in a fixed order (entry
 * e belongs to thread e mod 262144, a fixed butterfly over threads and workgroups, no atomics): bit-identical from run to
 * run and from device to device.
 *
 * Conventions of cumf_als_capi.h: DEVICE pointers of the calling process, `stream` a hipStream_t passed as void* (NULL =
 * the default stream), 0 on success or a HIP error code after printing the reason to stderr, no CPU fallback; a refused
 * call launches nothing.  Scope: even f >= 2 with a fused route at f + 2 (cumf_bias_available; in the default gram mode
 * f <= 204), lambda > 0 and lambda_bias > 0, one GPU.  Above that range there is no materialising fall-back.
 */
#ifndef CUMF_BIAS_CAPI_H_
#define CUMF_BIAS_CAPI_H_

#include "cumf_als_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CUMF_BIAS_SIDE_X 0     /* update XA from TA over the CSR rows: own bias in column f, the other in f + 1 */
#define CUMF_BIAS_SIDE_THETA 1 /* update TA from XA over the CSC columns: own bias in column f + 1, the other in f */

/* 1 when cumf_bias_update takes (f, solver): f even, f >= 2 and a fused route at f + 2.  Host only. */
int cumf_bias_available(int f, int solver);

/* One biased half-iteration (see above).  plan: made at f + 2; gather / update: the augmented tables (gather_rows x F and
 * the updated side's); gather_bias / own_bias: their bias vectors; sse_bins: NULL or CUMF_SSE_BINS doubles. */
int cumf_bias_update(const cumf_plan_t* plan, const int* colidx, const float* val, float* gather,
                     const float* gather_bias, float* update, float* own_bias, int f, int side, float mu, float lambda,
                     float lambda_bias, int solver, int cg_iters, double* sse_bins, void* stream);

/* Step 1 of cumf_bias_update on its own: out[e] = fl(fl(val[e] - mu) - bias[colidx[e]]) for `count` entries.  16-byte loads
 * and stores where val, colidx and out share their 16-byte phase, dword accesses for the head, the tail and otherwise. */
int cumf_bias_residual(const float* val, const int* colidx, long count, const float* bias, float mu, float* out,
                       void* stream);

/* out[e] = clamp(mu + score(rows[e], cols[e]), lo, hi) for `count` pairs; F is the tables' width f + 2. */
int cumf_bias_predict(const int* rows, const int* cols, long count, const float* XA, const float* TA, int F, float mu,
                      float lo, float hi, float* out, void* stream);

/* *out_f64 = sum over `count` entries of (val - prediction)^2, unclipped. */
int cumf_bias_sse(const float* val, const int* row, const int* col, long count, const float* XA, const float* TA, int F,
                  float mu, double* out_f64, void* stream);

/* *out_f64 = the mean of `count` values (0 for count == 0). */
int cumf_bias_mean(const float* val, long count, double* out_f64, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CUMF_BIAS_CAPI_H_ */
