/*
 * cumf_nnls_capi.h -- C ABI of the non-negative ALS of libALS.so (the `nonnegative` option of Spark MLlib's ALS).
 *
 * Problem.  For each materialised system (A: f x f fp32 symmetric positive definite, both triangles, row-major; b: f),
 *   x = argmin_{x >= 0} 1/2 x^T A x - b^T x,
 * i.e. the KKT point x >= 0, g = A x - b >= 0, x_i g_i = 0.  Solved by block principal pivoting (Kim & Park 2011) with
 * Murty's single-exchange backup rule; every passive-set solve is an unpivoted register LU of the masked system.
 *
 * Warm start.  x is read first: the initial passive set is {i : x_i > 0}.  x is then overwritten by the solution.  A and b
 * are only read.  With the support of the previous ALS iteration most rows need one solve.
 *
 * Convergence.  s = max|b| + max_i A_ii * max_{i passive}|x_i|, tol = f * 2^-24 * s: a row is converged when every passive
 * x_i >= -tol / max_i A_ii and every active g_i >= -tol.  The result is max(x, 0) on the passive set and 0 elsewhere, so
 * min x >= 0 holds exactly.
 *
 * max_iters: passive-set steps per row (one solve each; a step with an empty passive set needs none); 0 = the library
 * default, 16 + 2 f.  A row that reaches it returns its last iterate, clamped.  A row whose step is not finite (A not SPD:
 * a zero matrix, NaN) ends at once with x = 0.
 *
 * stats: NULL or 2 DEVICE int64 counters that are ADDED to: [0] rows not converged (cap reached or not finite), [1]
 * passive-set factorisations performed.
 *
 * Conventions of cumf_als_capi.h: DEVICE pointers of the calling process, `stream` a hipStream_t passed as void* (NULL = the
 * default stream), 0 on success or a HIP error code after printing the reason to stderr, no CPU fallback.  Plans are the
 * cumf_plan_t of cumf_als_capi.h (int32 or int64 row pointers).  Scope: the batched solver takes 1 <= f <= 128, the
 * half-iterations even 8 <= f <= 128 on one GPU; anything else is refused.  Every result is bit-identical from run to run
 * (fixed orders, integer atomics only).
 */
#ifndef CUMF_NNLS_CAPI_H_
#define CUMF_NNLS_CAPI_H_

#include "cumf_als_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when cumf_nnls_solve_batched takes f: 1 <= f <= 128.  Host only. */
int cumf_nnls_available(int f);

/* The NNLS solution of each of the `batch` systems (A: batch x f x f, b: batch x f) into x (batch x f; warm start in). */
int cumf_nnls_solve_batched(const float* A, const float* b, float* x, long batch, int f, int max_iters, long long* stats,
                            void* stream);

/* One explicit non-negative half-iteration over the plan's rows: the systems of cumf_get_hermitian (lambda n_u on the
 * diagonal, the current gram mode) solved by the NNLS solver with `update` (rows x f) as warm start and output.  Rows
 * without stored entries get x = 0 (their KKT point) without a factorisation. */
int cumf_als_update_nonneg(const cumf_plan_t* plan, const int* colidx, const float* val, const float* gather,
                           float* update, int f, float lambda, int max_iters, long long* stats, void* stream);

/* One implicit non-negative half-iteration: the systems of cumf_get_hermitian_implicit (G = cumf_implicit_gram of
 * `gather`; include/cumf_implicit_capi.h) solved by the NNLS solver; rows without stored entries get x = 0. */
int cumf_als_update_implicit_nonneg(const cumf_plan_t* plan, const int* colidx, const float* val, const float* gather,
                                    const float* G, float* update, int f, float lambda, float alpha, int reg_mode,
                                    int max_iters, long long* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CUMF_NNLS_CAPI_H_ */
