/*
 * cumf_free_capi.h -- C ABI of the matrix-free explicit-feedback half-iteration of libALS.so: explicit ALS at any even
 * 8 <= f <= 512 without ever forming a row's f x f system.
 *
 * Updating the rows X from the fixed table Y (n x f, `gather`), for a row u with n_u > 0 stored entries (i, r_ui):
 *   A_u = T_u^T T_u + reg_u I,   T_u = the n_u x f block of the gathered rows y_i,   reg_u = (float)n_u * lambda (fp32),
 *   b_u = T_u^T r_u,
 * the systems of cumf_get_hermitian, solved by the recurrence of cumf_cg_solve_batched: warm start from `update`, at most
 * cg_iters steps, a row ends when r.r < 1e-4 after a step and is frozen bit for bit from then on.  The kernels only
 * evaluate A_u v = T_u^T (T_u v) + reg_u v over the stored entries: cg_iters + 1 passes over the plan's entries, one gather
 * of each row's factor rows per pass, no f x f matrix anywhere (materialised, they are f^2 floats per row: 1 MB at f = 512).
 * Rows WITHOUT stored entries get x_u = 0, as the implicit and biased routes give them (cumf_get_hermitian +
 * cumf_cg_solve_batched return NaN there: 0 / 0 on the all-zero system).
 *
 * Conventions of cumf_als_capi.h: DEVICE pointers of the calling process, `stream` a hipStream_t passed as void* (NULL =
 * the default stream), 0 on success or a HIP error code after printing the reason to stderr, no CPU fallback.  Plans are the
 * cumf_plan_t of cumf_als_capi.h; a row's result does not depend on the plan's chunks, on the batch cuts or on the other
 * rows, and every result is bit-identical from run to run (fixed-order sums, no float atomics).
 * Scope: one GPU, the unbiased unconstrained model, CG only.  cumf_doALS_ex takes solver 2 (the value of
 * CUMF_SOLVER_CG_MATFREE in cumf_implicit_capi.h; environment CUMF_ALS_SOLVER=cg_matfree for doALS) and runs both
 * half-iterations here.  CUMF_SOLVER_CG keeps its routes at every f: cumf_fused_available(f, 2) stays 0.
 */
#ifndef CUMF_FREE_CAPI_H_
#define CUMF_FREE_CAPI_H_

#include "cumf_als_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 for even 8 <= f <= 512, else 0.  Host only: touches no device. */
int cumf_matfree_available(int f);

/* One half-iteration over the plan's rows at f = the plan's f; update (rows x f) is the CG warm start and receives the
 * solution.  The segment lists are built on the plan at its first call here (hence the non-const plan).  Refused with
 * hipErrorInvalidValue: a NULL plan or pointer, a plan whose f is odd, below 8 or above 512. */
int cumf_als_update_matfree(cumf_plan_t* plan, const int* colidx, const float* val, const float* gather, float* update,
                            float lambda, int cg_iters, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CUMF_FREE_CAPI_H_ */
