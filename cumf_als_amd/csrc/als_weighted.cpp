// als_weighted.cpp -- host side of weighted ALS (include/cumf_weighted_capi.h): the driver of als_free.cpp on the weighted
// kernels, the objective, and the C ABI.  Kernels: als_weighted.hip.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "als_weighted.h"
#include "cumf_implicit_capi.h"
#include "cumf_weighted_capi.h"

using namespace cumf;

namespace {

bool reg_mode_ok(int reg_mode) { return reg_mode == CUMF_IMPLICIT_REG_WEIGHTED || reg_mode == CUMF_IMPLICIT_REG_PLAIN; }
bool w0_ok(float w0) { return w0 >= 0.f; }  // false for NaN

}  // namespace

extern "C" int cumf_weighted_available(int f) { return matfree_f_ok(f); }

extern "C" int cumf_als_update_weighted(const cumf_plan_t* pc, const int* colidx, const float* val, const float* wgt,
                                        const float* gather, const float* G, float* update, float lambda, float w0,
                                        int reg_mode, int cg_iters, void* stream) {
  if (!pc || !colidx || !val || !wgt || !gather || !update) {
    fprintf(stderr, "cumf_als_update_weighted: plan, colidx, val, wgt, gather and update must not be NULL\n");
    return (int)hipErrorInvalidValue;
  }
  if (!matfree_f_ok(pc->f)) {
    fprintf(stderr, "cumf_als_update_weighted: needs a plan of even 8 <= f <= 512 (got %d)\n", pc->f);
    return (int)hipErrorInvalidValue;
  }
  if (!reg_mode_ok(reg_mode) || !w0_ok(w0)) {
    fprintf(stderr, "cumf_als_update_weighted: needs reg_mode 0 or 1 (got %d) and w0 >= 0 (got %g)\n", reg_mode, (double)w0);
    return (int)hipErrorInvalidValue;
  }
  if (w0 > 0.f && !G) {
    fprintf(stderr, "cumf_als_update_weighted: G must not be NULL when w0 > 0 (got w0 = %g)\n", (double)w0);
    return (int)hipErrorInvalidValue;
  }
  cumf_plan* p = const_cast<cumf_plan*>(pc);  // the segment lists are built on the plan at first use
  const hipStream_t s = static_cast<hipStream_t>(stream);
  ScratchLease lease;
  WeightedFreeArgs a{};
  a.G = G;
  a.reg_mode = reg_mode;
  a.wgt = wgt;
  a.w0 = w0;
  // the scratch of the explicit matrix-free route: the same three shapes, and calls on one stream are ordered
  return run_matfree(p, &a, colidx, val, gather, update, lambda, cg_iters, kScratchFreeVec, kScratchFreePart, kScratchFreeWords, s,
                     [&](int step, int steps) { return launch_weighted_free_pass(a, step, steps, s); });
}

extern "C" int cumf_weighted_gram(const float* table, const float* row_w, long rows, int f, float* G, void* stream) {
  if (!matfree_f_ok(f) || rows < 0 || !G || (rows > 0 && (!table || !row_w))) {
    fprintf(stderr, "cumf_weighted_gram: needs even 8 <= f <= 512 (got %d), rows >= 0 and table, row_w and G\n", f);
    return (int)hipErrorInvalidValue;
  }
  const hipStream_t s = static_cast<hipStream_t>(stream);
  ScratchLease lease;
  float* part = nullptr;
  int rc = scratch(s, kScratchImpGram, implicit_gram_part_floats(rows, f), &part);
  if (rc) return rc;
  CUMF_HIP_CHECK(launch_weighted_gram(table, row_w, rows, f, part, G, nullptr, s));
  return 0;
}

extern "C" int cumf_als_update_weighted_rank1(const cumf_plan_t* pc, const int* colidx, const float* val, const float* wgt,
                                              const float* gather, const float* G, const float* own_w0, const float* gather_w0,
                                              float* update, float lambda, int reg_mode, int cg_iters, void* stream) {
  if (!pc || !colidx || !val || !wgt || !gather || !G || !own_w0 || !gather_w0 || !update) {
    fprintf(stderr, "cumf_als_update_weighted_rank1: plan, colidx, val, wgt, gather, G, own_w0, gather_w0 and update must not "
                    "be NULL\n");
    return (int)hipErrorInvalidValue;
  }
  if (!matfree_f_ok(pc->f)) {
    fprintf(stderr, "cumf_als_update_weighted_rank1: needs a plan of even 8 <= f <= 512 (got %d)\n", pc->f);
    return (int)hipErrorInvalidValue;
  }
  if (!reg_mode_ok(reg_mode)) {
    fprintf(stderr, "cumf_als_update_weighted_rank1: needs reg_mode 0 or 1 (got %d)\n", reg_mode);
    return (int)hipErrorInvalidValue;
  }
  cumf_plan* p = const_cast<cumf_plan*>(pc);  // the segment lists are built on the plan at first use
  const hipStream_t s = static_cast<hipStream_t>(stream);
  ScratchLease lease;
  WeightedRank1Args a{};
  a.G = G;
  a.reg_mode = reg_mode;
  a.wgt = wgt;
  a.own_w0 = own_w0 + p->row_begin;  // the kernels index rows from the plan's first, as they do x
  a.gather_w0 = gather_w0;
  return run_matfree(p, &a, colidx, val, gather, update, lambda, cg_iters, kScratchFreeVec, kScratchFreePart, kScratchFreeWords, s,
                     [&](int step, int steps) { return launch_weighted_rank1_pass(a, step, steps, s); });
}

extern "C" int cumf_weighted_loss(const int* rowptr, const int* colidx, const float* val, const float* wgt, const float* XT,
                                  const float* thetaT, long m, long n, int f, float lambda, float w0, int reg_mode, double* out,
                                  void* stream) {
  if (!matfree_f_ok(f) || m < 0 || n < 0 || !out || !reg_mode_ok(reg_mode) || !w0_ok(w0)) {
    fprintf(stderr, "cumf_weighted_loss: needs even 8 <= f <= 512 (got %d), m, n >= 0, reg_mode 0 or 1, w0 >= 0 and out\n", f);
    return (int)hipErrorInvalidValue;
  }
  if ((m > 0 && (!rowptr || !XT)) || (n > 0 && !thetaT) || (m > 0 && n > 0 && (!colidx || !val || !wgt))) {
    fprintf(stderr, "cumf_weighted_loss: rowptr, colidx, val, wgt, XT and thetaT must not be NULL\n");
    return (int)hipErrorInvalidValue;
  }
  const hipStream_t s = static_cast<hipStream_t>(stream);
  ScratchLease lease;
  const size_t ff = (size_t)f * f;
  float* part = nullptr;
  double* aux = nullptr;  // Gx | Gy | loss partials (the scratch of cumf_implicit_loss: the same shapes)
  int rc = scratch(s, kScratchImpGram, std::max(implicit_gram_part_floats(m, f), implicit_gram_part_floats(n, f)), &part);
  if (!rc) rc = scratch(s, kScratchImpAux, 2 * ff + kImpLossBlocks, &aux);
  if (rc) return rc;
  CUMF_HIP_CHECK(launch_implicit_gram(XT, m, f, part, nullptr, aux, s));
  CUMF_HIP_CHECK(launch_implicit_gram(thetaT, n, f, part, nullptr, aux + ff, s));
  CUMF_HIP_CHECK(launch_weighted_loss(rowptr, colidx, val, wgt, XT, thetaT, m, f, lambda, w0, reg_mode, aux, aux + ff,
                                      aux + 2 * ff, out, s));
  return 0;
}

extern "C" int cumf_weighted_rank1_loss(const int* rowptr, const int* colidx, const float* val, const float* wgt, const float* XT,
                                        const float* thetaT, const float* row_w0, const float* col_w0, long m, long n, int f,
                                        float lambda, int reg_mode, double* out, void* stream) {
  if (!matfree_f_ok(f) || m < 0 || n < 0 || !out || !reg_mode_ok(reg_mode)) {
    fprintf(stderr, "cumf_weighted_rank1_loss: needs even 8 <= f <= 512 (got %d), m, n >= 0, reg_mode 0 or 1 and out\n", f);
    return (int)hipErrorInvalidValue;
  }
  if ((m > 0 && (!rowptr || !XT || !row_w0)) || (n > 0 && (!thetaT || !col_w0)) || (m > 0 && n > 0 && (!colidx || !val || !wgt))) {
    fprintf(stderr, "cumf_weighted_rank1_loss: rowptr, colidx, val, wgt, XT, thetaT, row_w0 and col_w0 must not be NULL\n");
    return (int)hipErrorInvalidValue;
  }
  const hipStream_t s = static_cast<hipStream_t>(stream);
  ScratchLease lease;
  const size_t ff = (size_t)f * f;
  float* part = nullptr;
  double* aux = nullptr;  // Gx | Gy | loss partials | the partials of the plain regulariser
  int rc = scratch(s, kScratchImpGram, std::max(implicit_gram_part_floats(m, f), implicit_gram_part_floats(n, f)), &part);
  if (!rc) rc = scratch(s, kScratchImpAux, 2 * ff + 2 * kImpLossBlocks, &aux);
  if (rc) return rc;
  CUMF_HIP_CHECK(launch_weighted_gram(XT, row_w0, m, f, part, nullptr, aux, s));
  CUMF_HIP_CHECK(launch_weighted_gram(thetaT, col_w0, n, f, part, nullptr, aux + ff, s));
  CUMF_HIP_CHECK(launch_weighted_rank1_loss(rowptr, colidx, val, wgt, XT, thetaT, row_w0, col_w0, m, n, f, lambda, reg_mode, aux,
                                            aux + ff, aux + 2 * ff, out, s));
  return 0;
}
