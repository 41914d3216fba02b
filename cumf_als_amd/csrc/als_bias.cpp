// als_bias.cpp -- host side of biased explicit ALS (include/cumf_bias_capi.h): the half-iteration as one call around the
// fused update of cumf_als_capi.h, prediction, the SSE and the mean.  Kernels: als_bias.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "als_bias.h"
#include "cumf_als_capi.h"
#include "cumf_bias_capi.h"

using namespace cumf;

extern "C" int cumf_bias_available(int f, int solver) {
  if (f < 2 || (f % 2) != 0) return 0;
  return cumf_fused_available(f + 2, solver);
}

extern "C" int cumf_bias_update(const cumf_plan_t* p, const int* colidx, const float* val, float* gather,
                                const float* gather_bias, float* update, float* own_bias, int f, int side, float mu,
                                float lambda, float lambda_bias, int solver, int cg_iters, double* sse_bins, void* stream) {
  // every refusal comes before the first launch
  if (!cumf_bias_available(f, solver)) {
    fprintf(stderr, "cumf_bias_update: f = %d with solver %d is outside the range of the biased half-iteration (even f >= 2 "
                    "with a fused route at f + 2, cumf_bias_available); there is no materialising path\n", f, solver);
    return (int)hipErrorInvalidValue;
  }
  const int F = f + 2;
  if (!p || p->f != F) {
    fprintf(stderr, "cumf_bias_update: the plan must be made at f + 2 = %d (got %d)\n", F, p ? p->f : 0);
    return (int)hipErrorInvalidValue;
  }
  if (side != CUMF_BIAS_SIDE_X && side != CUMF_BIAS_SIDE_THETA) {
    fprintf(stderr, "cumf_bias_update: side must be CUMF_BIAS_SIDE_X or CUMF_BIAS_SIDE_THETA (got %d)\n", side);
    return (int)hipErrorInvalidValue;
  }
  if (!(lambda > 0.f) || !(lambda_bias > 0.f) || !std::isfinite(lambda) || !std::isfinite(lambda_bias)) {
    fprintf(stderr, "cumf_bias_update: needs finite lambda > 0 and lambda_bias > 0 (got %g, %g)\n", lambda, lambda_bias);
    return (int)hipErrorInvalidValue;
  }
  if (p->gather_rows <= 0) {
    fprintf(stderr, "cumf_bias_update: needs the row count of the gather table (cumf_plan_set_gather_rows)\n");
    return (int)hipErrorInvalidValue;
  }
  if (!colidx || !val || !gather || !gather_bias || !update || !own_bias) {
    fprintf(stderr, "cumf_bias_update: null argument\n");
    return (int)hipErrorInvalidValue;
  }
  if (sse_bins && !cumf_fused_sse_available(p, solver)) {
    fprintf(stderr, "cumf_bias_update: the train SSE is not available for this plan (cumf_fused_sse_available)\n");
    return (int)hipErrorInvalidValue;
  }
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const float scale = (float)std::sqrt((double)lambda / (double)lambda_bias);
  const int own = side == CUMF_BIAS_SIDE_X ? f : f + 1, other = side == CUMF_BIAS_SIDE_X ? f + 1 : f;

  ScratchLease lease;  // the residual ratings stay ours until the fused update that reads them is enqueued
  // r' of the plan's entries [entry_begin, entry_begin + plan_nnz).  The fused kernels address ratings with the plan's own
  // entry offsets, so they get the pointer that entry 0 WOULD have; the buffer starts `skew` floats in, which gives entry e
  // of r' the 16-byte phase of entry e of val and lets the residual kernel move both with 16-byte accesses.
  const float* val0 = val + p->entry_begin;
  const size_t skew = (reinterpret_cast<uintptr_t>(val0) & 15) / sizeof(float);
  float* buf = nullptr;
  int rc = scratch(s, kScratchBiasResid, (size_t)p->plan_nnz + 4, &buf);
  if (rc) return rc;
  float* resid0 = buf + skew;
  CUMF_HIP_CHECK(launch_bias_residual(val0, colidx + p->entry_begin, gather_bias, mu, resid0, p->plan_nnz, s));
  CUMF_HIP_CHECK(launch_bias_columns(false, gather, gather_bias, p->gather_rows, update, own_bias, p->row_begin, p->row_end, F,
                                     own, other, scale, s));
  const float* resid = resid0 - (ptrdiff_t)p->entry_begin;
  rc = sse_bins ? cumf_als_update_fused_sse(p, colidx, resid, gather, update, F, lambda, solver, cg_iters, sse_bins, stream)
                : cumf_als_update_fused(p, colidx, resid, gather, update, F, lambda, solver, cg_iters, stream);
  // the tables go back to serving form whatever the fused call said: a failed call must not leave training columns behind
  CUMF_HIP_CHECK(launch_bias_columns(true, gather, gather_bias, p->gather_rows, update, own_bias, p->row_begin, p->row_end, F,
                                     own, other, scale, s));
  CUMF_HIP_CHECK(launch_bias_empty_rows(p->d_item_row, p->d_item_rowlen, p->n_items, update, own_bias, F, other, s));
  return rc;
}

extern "C" int cumf_bias_residual(const float* val, const int* colidx, long count, const float* bias, float mu, float* out,
                                  void* stream) {
  if (count < 0 || (count > 0 && (!val || !colidx || !bias || !out))) {
    fprintf(stderr, "cumf_bias_residual: needs count >= 0 and every array\n");
    return (int)hipErrorInvalidValue;
  }
  CUMF_HIP_CHECK(launch_bias_residual(val, colidx, bias, mu, out, count, static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int cumf_bias_predict(const int* rows, const int* cols, long count, const float* XA, const float* TA, int F,
                                 float mu, float lo, float hi, float* out, void* stream) {
  if (F <= 0 || count < 0 || (count > 0 && (!rows || !cols || !XA || !TA || !out))) {
    fprintf(stderr, "cumf_bias_predict: needs F >= 1 (got %d), count >= 0 and the tables\n", F);
    return (int)hipErrorInvalidValue;
  }
  CUMF_HIP_CHECK(launch_bias_predict(rows, cols, count, XA, TA, F, mu, lo, hi, out, static_cast<hipStream_t>(stream)));
  return 0;
}

namespace {
int bias_sum(const char* who, const float* val, const int* row, const int* col, long count, const float* XA, const float* TA,
             int F, float mu, double* out, void* stream) {
  if (!out || count < 0 || (count > 0 && !val)) {
    fprintf(stderr, "%s: needs count >= 0, the values and the output\n", who);
    return (int)hipErrorInvalidValue;
  }
  const hipStream_t s = static_cast<hipStream_t>(stream);
  ScratchLease lease;
  double* part = nullptr;
  const int rc = scratch(s, kScratchBiasPart, (size_t)kBiasSumBlocks, &part);
  if (rc) return rc;
  CUMF_HIP_CHECK(launch_bias_sum(val, row, col, count, XA, TA, F, mu, part, out, s));
  return 0;
}
}  // namespace

extern "C" int cumf_bias_sse(const float* val, const int* row, const int* col, long count, const float* XA, const float* TA,
                             int F, float mu, double* out_f64, void* stream) {
  if (F <= 0 || (count > 0 && (!row || !col || !XA || !TA))) {
    fprintf(stderr, "cumf_bias_sse: needs F >= 1 (got %d), the index arrays and the tables\n", F);
    return (int)hipErrorInvalidValue;
  }
  return bias_sum("cumf_bias_sse", val, row, col, count, XA, TA, F, mu, out_f64, stream);
}

extern "C" int cumf_bias_mean(const float* val, long count, double* out_f64, void* stream) {
  return bias_sum("cumf_bias_mean", val, nullptr, nullptr, count, nullptr, nullptr, 0, 0.f, out_f64, stream);
}
