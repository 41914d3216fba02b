/*
 * cumf_implicit_capi.h -- C ABI of the implicit-feedback ALS of libALS.so (Hu, Koren, Volinsky, "Collaborative
 * Filtering for Implicit Feedback Datasets", ICDM 2008; the `implicitPrefs` mode of Spark MLlib's ALS).
 *
 * A stored entry (u, i, r) has the confidence weight w = alpha |r| and the preference p = (r > 0); an unstored entry has
 * weight 0 (confidence 1) and preference 0.  Updating the rows X from the fixed table Y (n x f, `gather`):
 *   A_u = G + sum_{i in R(u)} w_ui y_i y_i^T + reg_u I,   G = Y^T Y over ALL rows of Y,
 *   b_u = sum_{i in R(u), r > 0} (1 + w_ui) y_i,
 * reg_u = lambda n_u (CUMF_IMPLICIT_REG_WEIGHTED, n_u = stored entries of row u) or lambda (CUMF_IMPLICIT_REG_PLAIN).
 * Rows without stored entries get x_u = 0.  The other side uses the same formulas on the CSC arrays.
 *
 * Conventions of cumf_als_capi.h: DEVICE pointers of the calling process, `stream` a hipStream_t passed as void* (NULL =
 * the default stream), 0 on success or a HIP error code after printing file/line to stderr, no CPU fallback.  Plans are
 * the cumf_plan_t of cumf_als_capi.h.  Scope: every entry point works on the calling process's GPU (several GPUs:
 * cumf_get_hermitian_implicit_partial + cumf_implicit_finish around the caller's own reduction, as
 * cumf_als_amd/dist_implicit.py does); even f with 8 <= f <= 512 for CUMF_SOLVER_CG_MATFREE, cumf_implicit_gram and
 * cumf_implicit_loss, even f with 8 <= f <= 128 for everything else; anything else is refused.
 * Every result is bit-identical from run to run (fixed-order reductions, no float atomics).
 */
#ifndef CUMF_IMPLICIT_CAPI_H_
#define CUMF_IMPLICIT_CAPI_H_

#include "cumf_als_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { CUMF_IMPLICIT_REG_WEIGHTED = 0, CUMF_IMPLICIT_REG_PLAIN = 1 };

/* The third implicit solver (after CUMF_SOLVER_CG = 0 and CUMF_SOLVER_LU = 1 of cumf_als_capi.h); implicit entry points only. */
enum { CUMF_SOLVER_CG_MATFREE = 2 };

/* 1 when the implicit entry points take (f, solver): even f in [8, 128] with CUMF_SOLVER_CG or CUMF_SOLVER_LU, even f in
 * [8, 512] with CUMF_SOLVER_CG_MATFREE. */
int cumf_implicit_available(int f, int solver);

/* G = table^T table of a rows x f fp32 table (even 8 <= f <= 512): f x f fp32, both triangles, exactly symmetric.  fp32
 * matrix-pipe products per slab of rows (1 024 rows up to f = 128, more above), the slab partials summed in slab order
 * in fp64. */
int cumf_implicit_gram(const float* table, long rows, int f, float* G, void* stream);

/* The materialised systems of the plan's rows: tt receives (row_end - row_begin) x f x f fp32 (row-major, both
 * triangles; the layout of cumf_get_hermitian), rhs (row_end - row_begin) x f.  G: the f x f Gram of `gather`
 * (cumf_implicit_gram).  Rows cut into chunks by the plan are summed over per-chunk partials in chunk order. */
int cumf_get_hermitian_implicit(const cumf_plan_t* plan, const int* colidx, const float* val, const float* gather,
                                const float* G, float* tt, float* rhs, int f, float lambda, float alpha, int reg_mode,
                                void* stream);

/* The PARTIAL systems of the plan's rows over the stored entries of THIS plan alone -- what one rank of a multi-GPU run
 * contributes when the gather table is row-sharded (the plan over the slab-local CSC, `gather` the slab of the table):
 *   packed[row - row_begin]  f (f + 1) / 2 floats, the upper triangle in row-major order (the layout of
 *                            cumf_get_hermitian_packed): sum over the plan's entries of w y y^T, plus lambda n_local on the
 *                            diagonal with CUMF_IMPLICIT_REG_WEIGHTED (n_local = the row's entries in this plan); nothing
 *                            is added with CUMF_IMPLICIT_REG_PLAIN;
 *   rhs[row - row_begin]     f floats: sum_{r > 0} (1 + w) y.
 * G is not added and not read: the partials of the ranks sum to the full system minus G (and minus lambda I in plain
 * mode), which cumf_implicit_finish completes.  A row without entries in this plan gets all-zero output, written by the
 * kernel itself (a plan lists every row of its batch).  Rows cut into chunks are summed over per-chunk partials in chunk
 * order in fp64, as in cumf_get_hermitian_implicit.  The same accumulation as cumf_get_hermitian_implicit: only the
 * epilogue differs.  Even 8 <= f <= 128. */
int cumf_get_hermitian_implicit_partial(const cumf_plan_t* plan, const int* colidx, const float* val, const float* gather,
                                        float* packed, float* rhs, int f, float lambda, float alpha, int reg_mode,
                                        void* stream);

/* Summed partials -> solvable systems: for every b < batch and i, j < f, in this order of fp32 operations,
 *   t        = packed[b][(min(i, j), max(i, j))] + G[i][j]      one fp32 addition
 *   tt[b][i][j] = (i == j) ? t + reg_add : t                      a second fp32 addition on the diagonal
 * tt: batch x f x f, both triangles; exactly symmetric when G is (cumf_implicit_gram's is; so is a sum of them).
 * reg_add: lambda with CUMF_IMPLICIT_REG_PLAIN, 0 with CUMF_IMPLICIT_REG_WEIGHTED (whose partials carry lambda n already).
 * Even 8 <= f <= 128. */
int cumf_implicit_finish(const float* packed, const float* G, float reg_add, float* tt, long batch, int f, void* stream);

/* One implicit half-iteration over the plan's rows; update (rows x f) is the CG warm start and receives the solution.
 *   CUMF_SOLVER_CG: rows of at most 32 stored entries run a CG that never forms A_u (A p = G p + T^T (w o T p) + reg p,
 *                   T the row's gathered block); longer rows are materialised and solved by cumf_cg_solve_batched.  The
 *                   recurrence of cumf_cg_solve_batched: warm start, at most cg_iters steps, exit when r.r < 1e-4.
 *   CUMF_SOLVER_LU: every row materialised and solved by cumf_lu_solve_batched.
 *   CUMF_SOLVER_CG_MATFREE (even 8 <= f <= 512): no row forms A_u; every step evaluates A p = G p + T^T (w o T p) + reg p
 *                   over the stored entries and G.  The same recurrence, checked per row.
 * Rows without stored entries are set to 0 by all three. */
int cumf_als_update_implicit(const cumf_plan_t* plan, const int* colidx, const float* val, const float* gather,
                             const float* G, float* update, int f, float lambda, float alpha, int reg_mode, int solver,
                             int cg_iters, void* stream);

/* The implicit objective into *out (one DEVICE double):
 *   L = sum_{all u,i} c_ui (p_ui - x_u.y_i)^2 + sum_u reg_u |x_u|^2 + sum_i reg_i |y_i|^2
 *     = <X^T X, Y^T Y>_F + sum_stored [(1 + w)(p - s)^2 - s^2] + regs,   s = x_u.y_i,
 * from the CSR arrays of the ratings (rowptr: m + 1 ints), XT (m x f) and thetaT (n x f), fp64 accumulation. */
int cumf_implicit_loss(const int* rowptr, const int* colidx, const float* val, const float* XT, const float* thetaT,
                       long m, long n, int f, float lambda, float alpha, int reg_mode, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CUMF_IMPLICIT_CAPI_H_ */
