/*
 * cumf_weighted_capi.h -- C ABI of the weighted ALS of libALS.so: a weight on every stored entry and one weight on
 * everything unstored (or, at the end of this file, a rank-one weight a_u c_i on the unstored entry (u, i)), at any even
 * 8 <= f <= 512, without ever forming a row's f x f system.
 *
 * A stored entry (u, i) has the rating r_ui and the weight w_ui >= 0; every unstored entry has the target 0 and the weight
 * w0 >= 0.  The objective is
 *   L = sum_stored w_ui (r_ui - x_u . y_i)^2 + w0 sum_unstored (x_u . y_i)^2 + sum_u reg_u |x_u|^2 + sum_i reg_i |y_i|^2,
 * reg_u = lambda n_u (CUMF_IMPLICIT_REG_WEIGHTED of cumf_implicit_capi.h; n_u = the stored entries of row u, those of weight 0
 * included) or lambda (CUMF_IMPLICIT_REG_PLAIN).  Updating the rows X from the fixed table Y (n x f, `gather`):
 *   A_u = w0 G + sum_{i in R(u)} (w_ui - w0) y_i y_i^T + reg_u I,   G = Y^T Y over ALL rows of Y,
 *   b_u = sum_{i in R(u)} w_ui r_ui y_i.
 * A_u is symmetric positive definite for any w >= 0, w0 >= 0 (it is w0 sum_unstored y y^T + sum_stored w y y^T + reg I), and
 * is solved by the recurrence of cumf_cg_solve_batched: warm start from `update`, at most cg_iters steps, a row ends when
 * r.r < 1e-4 after a step and is frozen bit for bit from then on.  The kernels only evaluate
 *   A_u v = w0 (G v) + T_u^T ((w - w0) o (T_u v)) + reg_u v
 * (T_u = the n_u x f block of the gathered rows): cg_iters + 1 passes over the plan's entries, G v on the matrix pipe for 32
 * rows at a time.  Rows WITHOUT stored entries get x_u = 0, their exact minimiser (b_u = 0).  The other side uses the same
 * formulas on the CSC arrays, with the weights in CSC order.
 *
 * Two special cases, bit for bit: w = 1, w0 = 0, CUMF_IMPLICIT_REG_WEIGHTED is cumf_als_update_matfree (cumf_free_capi.h);
 * w = 1 + alpha |r|, val = (r > 0), w0 = 1 is cumf_als_update_implicit with CUMF_SOLVER_CG_MATFREE wherever w - 1 and
 * w val are exact in fp32.
 *
 * Conventions of cumf_als_capi.h: DEVICE pointers of the calling process, `stream` a hipStream_t passed as void* (NULL =
 * the default stream), 0 on success or a HIP error code after printing the reason to stderr, no CPU fallback.  Plans are the
 * cumf_plan_t of cumf_als_capi.h; a row's result does not depend on the plan's chunks, on the batch cuts or on the other
 * rows, and every result is bit-identical from run to run (fixed-order sums, no float atomics).
 * Scope: one GPU, CG only, the unbiased unconstrained model.  Not covered: LU or any materialised weighted system, a
 * regulariser lambda sum_i w_ui, biases or non-negativity combined with weights, cumf_doALS, several GPUs.
 */
#ifndef CUMF_WEIGHTED_CAPI_H_
#define CUMF_WEIGHTED_CAPI_H_

#include "cumf_als_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 for even 8 <= f <= 512, else 0.  Host only: touches no device. */
int cumf_weighted_available(int f);

/* One half-iteration over the plan's rows at f = the plan's f; update (rows x f) is the CG warm start and receives the
 * solution.  wgt: the weight of each stored entry, indexed as val (w >= 0 is the caller's contract: the array is not
 * scanned).  G: cumf_implicit_gram(gather), read only when w0 > 0 and may be NULL when w0 == 0.  The segment lists are built
 * on the plan at its first matrix-free call.  Refused with hipErrorInvalidValue before any device call: a NULL plan or
 * pointer, a plan whose f is odd, below 8 or above 512, an unknown reg_mode, w0 < 0 or NaN, G == NULL with w0 > 0. */
int cumf_als_update_weighted(const cumf_plan_t* plan, const int* colidx, const float* val, const float* wgt,
                             const float* gather, const float* G, float* update, float lambda, float w0, int reg_mode,
                             int cg_iters, void* stream);

/* The objective L above of the factors XT (m x f) and thetaT (n x f) on the CSR arrays rowptr (m + 1, int32) / colidx / val /
 * wgt, as one fp64 value in out[0] (device).  Evaluated as
 *   w0 (<X^T X, Y^T Y>_F - sum_stored s^2) + sum_stored w (r - s)^2 + regs,   s = x_u . y_i,
 * in fp64 with fixed-order sums (the fp64 Grams of cumf_implicit_gram's partials): O(nnz f + (m + n) f^2), never m x n. */
int cumf_weighted_loss(const int* rowptr, const int* colidx, const float* val, const float* wgt, const float* XT,
                       const float* thetaT, long m, long n, int f, float lambda, float w0, int reg_mode, double* out,
                       void* stream);

/* ---- Rank-one weights on the unstored entries: the unstored entry (u, i) weighs a_u c_i (a >= 0 of length m, c >= 0 of length
 * n) in place of the one scalar w0 -- eALS's popularity weights c_i = c0 n_i^e / sum_j n_j^e (He et al., SIGIR 2016) with a = 1,
 * per-user exposure weights with c = 1, w0 itself with a = w0, c = 1.
 *   L = sum_stored w (r - x_u . y_i)^2 + sum_unstored a_u c_i (x_u . y_i)^2 + sum_u reg_u |x_u|^2 + sum_i reg_i |y_i|^2,
 *   A_u = a_u G_c + sum_{i in R(u)} (w_ui - a_u c_i) y_i y_i^T + reg_u I,   G_c = Y^T diag(c) Y,   b_u = sum w r y,
 * and the mirror image on the other side (A_i = c_i G_a + sum (w - a_u c_i) x x^T + reg_i I, G_a = X^T diag(a) X).  A
 * half-iteration therefore takes an OWN weight vector, indexed as the rows of `update`, and a GATHER weight vector, indexed
 * as the rows of `gather`; G is the Gram of `gather` weighted by the gather vector.  A_u = a_u sum_unstored c y y^T +
 * sum_stored w y y^T + reg I is positive definite although w - a_u c_i may be negative.  The kernels evaluate
 *   A_u v = a_u (G_c v) + T_u^T ((w - a_u c) o (T_u v)) + reg_u v:
 * per stored entry and pass one more 4-byte gather (c_i, by the column index already held) than cumf_als_update_weighted, and
 * one scale per row of G_c v.  With gather_w0 = 1 and own_w0 = w0 every pass returns the bits of cumf_als_update_weighted. */

/* G = sum_k row_w[k] y_k y_k^T (f x f fp32, both triangles, exactly symmetric) of the rows x f table: cumf_implicit_gram with
 * the weight of table row k on one operand -- the same slabs, stages, tile order and fp64 slab reduction; with row_w = 1 its
 * bits.  row_w >= 0 and finite is the caller's contract.  Refused with hipErrorInvalidValue: f odd, below 8 or above 512,
 * rows < 0, a NULL G, a NULL table or row_w with rows > 0. */
int cumf_weighted_gram(const float* table, const float* row_w, long rows, int f, float* G, void* stream);

/* cumf_als_update_weighted with the weight own_w0[u] gather_w0[i] on the unstored entry (u, i).  own_w0: one weight per row of
 * `update` (ALL its rows, indexed by absolute row whatever rows the plan covers); gather_w0: one per row of `gather`; G:
 * cumf_weighted_gram(gather, gather_w0).  The weights are the caller's contract (>= 0, finite) and are not scanned.  Refused
 * with hipErrorInvalidValue before any device call: a NULL plan or pointer (G, own_w0 and gather_w0 are all required), a plan
 * whose f is odd, below 8 or above 512, an unknown reg_mode. */
int cumf_als_update_weighted_rank1(const cumf_plan_t* plan, const int* colidx, const float* val, const float* wgt,
                                   const float* gather, const float* G, const float* own_w0, const float* gather_w0,
                                   float* update, float lambda, int reg_mode, int cg_iters, void* stream);

/* The objective L above on the CSR arrays, row_w0 = a (m) and col_w0 = c (n), as one fp64 value in out[0] (device).  Evaluated as
 *   sum_stored [w (r - s)^2 - a_u c_i s^2] + <X^T diag(a) X, Y^T diag(c) Y>_F + regs,   s = x_u . y_i,
 * in fp64 with fixed-order sums (the fp64 output of cumf_weighted_gram's reduction): never m x n. */
int cumf_weighted_rank1_loss(const int* rowptr, const int* colidx, const float* val, const float* wgt, const float* XT,
                             const float* thetaT, const float* row_w0, const float* col_w0, long m, long n, int f,
                             float lambda, int reg_mode, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CUMF_WEIGHTED_CAPI_H_ */
