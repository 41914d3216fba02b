// als_bias.h -- biased explicit ALS (include/cumf_bias_capi.h): what als_bias.cpp (host side) takes from als_bias.hip (the
// kernels around the fused half-iteration: residual ratings, the bias columns of the augmented tables, prediction, SSE, mean).
#ifndef CUMF_ALS_BIAS_H_
#define CUMF_ALS_BIAS_H_

#include "als_internal.h"

namespace cumf {

// Workgroups of the fp64 reductions (SSE, mean): a constant, so that the order of the sum -- and with it every bit of the
// result -- depends on neither the device nor the run.  `part` of the launchers below: kBiasSumBlocks doubles.
constexpr int kBiasSumBlocks = 1024;
constexpr int kBiasThreads = 256;

// out[e] = (val[e] - mu) - bias[colidx[e]] for e in [0, count): fp32, two roundings.  16-byte loads and stores where val,
// colidx and out are aligned alike (the caller offsets `out` to make it so), dword accesses for the head, the tail and
// everything else.
hipError_t launch_bias_residual(const float* val, const int* colidx, const float* bias, float mu, float* out,
                                long long count, hipStream_t stream);
// The two bias columns of the augmented tables, before (training form) and after (serving form) the fused update; `own` is
// the column of the updated side's bias, `other` the column of the gathered side's.
//   training: gather[:, own] = s, gather[:, other] = 0; update[u, own] = own_bias[u] / s, update[u, other] = 0
//   serving:  own_bias[u] = update[u, own] * s; update[u, own] = own_bias[u], update[u, other] = 1;
//             gather[:, own] = 1, gather[:, other] = gather_bias
// for every row of the gather table and the rows u in [row_begin, row_end) of the update table.
hipError_t launch_bias_columns(bool serving, float* gather, const float* gather_bias, long gather_rows, float* update,
                               float* own_bias, long row_begin, long row_end, int F, int own, int other, float s,
                               hipStream_t stream);
// Rows without ratings (items of row length 0): update[u, 0 .. F) = 0 except column `other` (kept), own_bias[u] = 0
hipError_t launch_bias_empty_rows(const int* item_row, const int* item_rowlen, long n_items, float* update, float* own_bias,
                                  int F, int other, hipStream_t stream);
// out[e] = clamp(mu + chain(XA[rows[e]], TA[cols[e]]), lo, hi); NaN stays NaN
hipError_t launch_bias_predict(const int* rows, const int* cols, long long count, const float* XA, const float* TA, int F,
                               float mu, float lo, float hi, float* out, hipStream_t stream);
// *out = sum (val - prediction)^2 (row != nullptr) or the mean of val (row == nullptr), fp64 in a fixed order
hipError_t launch_bias_sum(const float* val, const int* row, const int* col, long long count, const float* XA,
                           const float* TA, int F, float mu, double* part, double* out, hipStream_t stream);

}  // namespace cumf

#endif  // CUMF_ALS_BIAS_H_
