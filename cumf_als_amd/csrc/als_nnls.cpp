// als_nnls.cpp -- host side of non-negative ALS (include/cumf_nnls_capi.h): the batched NNLS solver and the two
// half-iteration routes that feed it materialised systems.  Kernel: als_nnls.hip.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "als_implicit.h"
#include "als_nnls.h"
#include "cumf_als_capi.h"
#include "cumf_implicit_capi.h"
#include "cumf_nnls_capi.h"

using namespace cumf;

namespace {

bool nnls_f_ok(int f) { return f >= 1 && f <= kNnlsMaxF; }
bool route_f_ok(int f) { return f >= 8 && f <= kNnlsMaxF && (f % 2) == 0; }
int cap_of(int f, int max_iters) { return max_iters > 0 ? max_iters : kNnlsDefaultItersBase + 2 * f; }

int check_route(const char* who, const cumf_plan_t* p, int f, int max_iters) {
  if (!p || f != p->f || !route_f_ok(f) || max_iters < 0) {
    fprintf(stderr, "%s: needs a plan of the same f, even 8 <= f <= %d (got %d) and max_iters >= 0 (got %d)\n", who,
            kNnlsMaxF, f, max_iters);
    return (int)hipErrorInvalidValue;
  }
  return 0;
}

// The tail both routes share, on the plan's materialised systems tt / rhs (indexed by row - row_begin): the rows without
// stored entries get x = 0 and b = 0 first, which is their KKT point (A x - b = 0), so the solver leaves them at 0 without a
// factorisation; then every row is solved with `update` as warm start and output.
int solve_plan_rows(cumf_plan* p, float* tt, float* rhs, float* update, int f, int max_iters, long long* stats,
                    hipStream_t s) {
  const int* empty = nullptr;
  long n_empty = 0;
  int rc = plan_empty_rows(p, &empty, &n_empty);
  if (rc) return rc;
  CUMF_HIP_CHECK(launch_implicit_zero_rows(empty, n_empty, f, update, s));
  CUMF_HIP_CHECK(launch_implicit_zero_rows(empty, n_empty, f, rhs - (ptrdiff_t)p->row_begin * f, s));
  const long rows = p->row_end - p->row_begin;
  CUMF_HIP_CHECK(launch_nnls(tt, rhs, update + (size_t)p->row_begin * f, rows, f, cap_of(f, max_iters), stats, s));
  return 0;
}

}  // namespace

extern "C" int cumf_nnls_available(int f) { return nnls_f_ok(f); }

extern "C" int cumf_nnls_solve_batched(const float* A, const float* b, float* x, long batch, int f, int max_iters,
                                       long long* stats, void* stream) {
  if (!nnls_f_ok(f) || batch < 0 || max_iters < 0 || (batch > 0 && (!A || !b || !x))) {
    fprintf(stderr, "cumf_nnls_solve_batched: needs 1 <= f <= %d (got %d), batch >= 0 and max_iters >= 0\n", kNnlsMaxF, f);
    return (int)hipErrorInvalidValue;
  }
  CUMF_HIP_CHECK(launch_nnls(A, b, x, batch, f, cap_of(f, max_iters), stats, static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int cumf_als_update_nonneg(const cumf_plan_t* pc, const int* colidx, const float* val, const float* gather,
                                      float* update, int f, float lambda, int max_iters, long long* stats, void* stream) {
  int rc = check_route("cumf_als_update_nonneg", pc, f, max_iters);
  if (rc) return rc;
  cumf_plan* p = const_cast<cumf_plan*>(pc);  // the empty-row list is built on the plan at first use
  const hipStream_t s = static_cast<hipStream_t>(stream);
  ScratchLease lease;
  const long rows = p->row_end - p->row_begin;
  float *tt = nullptr, *rhs = nullptr;
  if ((rc = scratch(s, kScratchNnlsTT, (size_t)rows * f * f, &tt)) || (rc = scratch(s, kScratchNnlsRhs, (size_t)rows * f, &rhs)))
    return rc;
  // lambda n_u on the diagonal, the Gram arithmetic of the current gram mode
  if ((rc = cumf_get_hermitian(p, colidx, val, gather, tt, rhs, f, lambda, stream))) return rc;
  return solve_plan_rows(p, tt, rhs, update, f, max_iters, stats, s);
}

extern "C" int cumf_als_update_implicit_nonneg(const cumf_plan_t* pc, const int* colidx, const float* val,
                                               const float* gather, const float* G, float* update, int f, float lambda,
                                               float alpha, int reg_mode, int max_iters, long long* stats, void* stream) {
  int rc = check_route("cumf_als_update_implicit_nonneg", pc, f, max_iters);
  if (rc) return rc;
  cumf_plan* p = const_cast<cumf_plan*>(pc);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  ScratchLease lease;
  const long rows = p->row_end - p->row_begin;
  float *tt = nullptr, *rhs = nullptr;
  if ((rc = scratch(s, kScratchNnlsTT, (size_t)rows * f * f, &tt)) || (rc = scratch(s, kScratchNnlsRhs, (size_t)rows * f, &rhs)))
    return rc;
  // every row materialised, as the LU route of cumf_als_update_implicit does (it refuses a bad reg_mode)
  if ((rc = cumf_get_hermitian_implicit(p, colidx, val, gather, G, tt, rhs, f, lambda, alpha, reg_mode, stream))) return rc;
  return solve_plan_rows(p, tt, rhs, update, f, max_iters, stats, s);
}
