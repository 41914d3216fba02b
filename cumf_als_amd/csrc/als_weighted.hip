// als_weighted.hip -- weighted ALS at any even 8 <= f <= 512: per-entry weights w >= 0 on the stored entries and one weight
// w0 >= 0 on every unstored entry (target 0), by the operator-only ("matrix-free") CG of include/cumf_weighted_capi.h.
//
// The CG never forms A_u.  Each step needs, for every live row u, A_u v = w0 (G v) + T_u^T ((w - w0) o (T_u v)) + reg_u v
// (T_u the row's gathered block of factor rows): the core of als_free_core.h with the weights taken from an array.
//   weighted_free_sparse_kernel  one wave per segment of a row (free_sparse_pass); b = sum w r y;
//   weighted_free_row_kernel     w0 = 0: one wave per row (free_row_update), no G, no LDS;
//   weighted_gram_row_kernel     w0 > 0: kFreeRows rows per workgroup with G v on v_mfma_f32_16x16x4_f32 (free_gram_rows),
//                                G v scaled by w0 as it leaves the accumulators;
//   weighted_loss_*              the objective from the stored entries and two fp64 Grams;
//   weighted_rank1_sparse_kernel, weighted_rank1_row_kernel, weighted_rank1_loss_*
//                                the same three with the weight a_u c_i on the unstored entry (u, i) (als_weighted.h): the
//                                sparse pass gathers c_i by the column index it holds, the row pass scales row u of G_c v by
//                                a_u.  With c = 1 and a = w0 every pass is the one above, bit for bit.
// With w = 1, w0 = 0 every product with a weight is the other factor itself and the passes are those of als_free.hip bit for
// bit; with w0 = 1 and weights for which w - 1 and w r are exact they are those of als_implicit_free.hip.  A row's result
// depends on its own entries, weights, warm start, f, lambda, w0, the reg mode and cg_iters only.
#include <hip/hip_runtime.h>

#include "als_free_core.h"
#include "als_loss.h"
#include "als_weighted.h"

namespace cumf {

template <int Q>
__global__ __launch_bounds__(kFreeThreads) void weighted_free_sparse_kernel(const WeightedFreeArgs a, int first) {
  free_sparse_pass<Q, kFreeWeightArray>(a, first, a.w0, a.wgt);
}

template <int Q>
__global__ __launch_bounds__(kFreeThreads) void weighted_free_row_kernel(const WeightedFreeArgs a, int mode, int last) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long row = (long long)blockIdx.x * 4 + wave;
  if (row >= a.rows || a.done[row]) return;  // uniform
  const int n = a.row_len[row];
  const float reg = a.reg_mode == kImpRegPlain ? a.lambda : (float)n * a.lambda;
  free_row_update<Q, false>(a, row, n, reg, nullptr, lane, mode, last);
}

template <int Q>
__global__ __launch_bounds__(kFreeThreads) void weighted_gram_row_kernel(const WeightedFreeArgs a, int mode, int last) {
  free_gram_rows<Q, kFreeScaleScalar>(a, a.w0, mode, last);
}

template <int Q>
__global__ __launch_bounds__(kFreeThreads) void weighted_rank1_sparse_kernel(const WeightedRank1Args a, int first) {
  free_sparse_pass<Q, kFreeWeightRank1>(a, first, 0.f, a.wgt, a.own_w0, a.gather_w0);
}

template <int Q>
__global__ __launch_bounds__(kFreeThreads) void weighted_rank1_row_kernel(const WeightedRank1Args a, int mode, int last) {
  free_gram_rows<Q, kFreeScaleRow>(a, 1.f, mode, last, a.own_w0);
}

hipError_t launch_weighted_free_pass(const WeightedFreeArgs& a, int step, int cg_iters, hipStream_t stream) {
  const int Q = (a.f + 63) / 64;
  const int first = step == 0, last = step >= cg_iters;
  if (a.rows <= 0 || a.rows > (1ll << 32)) return a.rows ? hipErrorInvalidValue : hipSuccess;  // no stride over the rows
  return with_nb<1, 8>(Q, [&](auto qc) {
    constexpr int QC = decltype(qc)::value;
    hipError_t e = hipSuccess;
    if (a.nseg > 0)
      e = launch_kernel(weighted_free_sparse_kernel<QC>, dim3(free_grid(a.nseg, 4, 16384)), dim3(kFreeThreads), 0, stream, a,
                        first);
    if (e != hipSuccess) return e;
    if (a.w0 > 0.f)
      return launch_item_kernel(weighted_gram_row_kernel<QC>, dim3(free_grid(a.rows, kFreeRows, 1ll << 30)), dim3(kFreeThreads),
                                0, stream, a, first ? 0 : 1, last);
    return launch_item_kernel(weighted_free_row_kernel<QC>, dim3(free_grid(a.rows, 4, 1ll << 30)), dim3(kFreeThreads), 0, stream,
                              a, first ? 0 : 1, last);
  });
}

hipError_t launch_weighted_rank1_pass(const WeightedRank1Args& a, int step, int cg_iters, hipStream_t stream) {
  const int Q = (a.f + 63) / 64;
  const int first = step == 0, last = step >= cg_iters;
  if (a.rows <= 0 || a.rows > (1ll << 32)) return a.rows ? hipErrorInvalidValue : hipSuccess;  // no stride over the rows
  return with_nb<1, 8>(Q, [&](auto qc) {
    constexpr int QC = decltype(qc)::value;
    hipError_t e = hipSuccess;
    if (a.nseg > 0)
      e = launch_kernel(weighted_rank1_sparse_kernel<QC>, dim3(free_grid(a.nseg, 4, 16384)), dim3(kFreeThreads), 0, stream, a,
                        first);
    if (e != hipSuccess) return e;
    return launch_item_kernel(weighted_rank1_row_kernel<QC>, dim3(free_grid(a.rows, kFreeRows, 1ll << 30)), dim3(kFreeThreads),
                              0, stream, a, first ? 0 : 1, last);
  });
}

// ---- the objective
//   L = w0 (<X^T X, Y^T Y>_F - sum_stored s^2) + sum_stored w (r - s)^2 + regs,  s = x_u . y_i,
// in fp64: kImpLossBlocks partials over the stored entries (the pass of als_loss.h, shared with the implicit objective),
// summed in a fixed order by one workgroup that adds the Gram term.

// part[block] = sum over its rows' stored entries of w (r - s)^2 - w0 s^2 (+ lambda (|x_u|^2 + |y_i|^2) when the regulariser
// is weighted): the pass of als_loss.h, shared with the implicit objective (als_implicit.hip)
__global__ __launch_bounds__(kLossThreads) void weighted_loss_kernel(const int* __restrict__ rowptr,
                                                                     const int* __restrict__ colidx,
                                                                     const float* __restrict__ val,
                                                                     const float* __restrict__ wgt,
                                                                     const float* __restrict__ XT,
                                                                     const float* __restrict__ thetaT, long long m, int f,
                                                                     float lambda, float w0, int reg_mode,
                                                                     double* __restrict__ part) {
  const double w0d = w0;
  loss_sparse_pass(rowptr, colidx, XT, thetaT, m, f, lambda, reg_mode != kImpRegPlain, part, [&](long long k, double s) {
    const double r = val[k], w = wgt[k];
    return w * (r - s) * (r - s) - w0d * s * s;
  });
}

// out = sum of the parts + w0 <Gx, Gy>_F (+ lambda (tr Gx + tr Gy) when the regulariser is plain)
__global__ __launch_bounds__(kLossThreads) void weighted_loss_final_kernel(const double* __restrict__ part, int nparts,
                                                                           const double* __restrict__ Gx,
                                                                           const double* __restrict__ Gy, int f, float lambda,
                                                                           float w0, int reg_mode, double* __restrict__ out) {
  __shared__ double red[kLossThreads];
  double acc = 0.0, gg = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kLossThreads) acc += part[i];
  for (int e = threadIdx.x; e < f * f; e += kLossThreads) gg += Gx[e] * Gy[e];
  acc += (double)w0 * gg;
  if (reg_mode == kImpRegPlain)
    for (int i = threadIdx.x; i < f; i += kLossThreads) acc += (double)lambda * (Gx[i * f + i] + Gy[i * f + i]);
  const double t = loss_block_sum(acc, red);
  if (threadIdx.x == 0) out[0] = t;
}

hipError_t launch_weighted_loss(const int* rowptr, const int* colidx, const float* val, const float* wgt, const float* XT,
                                const float* thetaT, long m, int f, float lambda, float w0, int reg_mode, const double* Gx,
                                const double* Gy, double* part, double* out, hipStream_t stream) {
  hipError_t e = launch_kernel(weighted_loss_kernel, dim3(kImpLossBlocks), dim3(kLossThreads), 0, stream, rowptr, colidx, val,
                               wgt, XT, thetaT, (long long)m, f, lambda, w0, reg_mode, part);
  if (e != hipSuccess) return e;
  return launch_kernel(weighted_loss_final_kernel, dim3(1), dim3(kLossThreads), 0, stream, (const double*)part,
                       (int)kImpLossBlocks, Gx, Gy, f, lambda, w0, reg_mode, out);
}

// ---- the rank-one objective
//   L = sum_stored [w (r - s)^2 - a_u c_i s^2] + <X^T diag(a) X, Y^T diag(c) Y>_F + regs,  s = x_u . y_i

// part[block] = sum over its rows' stored entries of w (r - s)^2 - a_u c_i s^2 (+ lambda (|x_u|^2 + |y_i|^2) when the
// regulariser is weighted)
__global__ __launch_bounds__(kLossThreads) void weighted_rank1_loss_kernel(const int* __restrict__ rowptr,
                                                                           const int* __restrict__ colidx,
                                                                           const float* __restrict__ val,
                                                                           const float* __restrict__ wgt,
                                                                           const float* __restrict__ XT,
                                                                           const float* __restrict__ thetaT,
                                                                           const float* __restrict__ row_w0,
                                                                           const float* __restrict__ col_w0, long long m, int f,
                                                                           float lambda, int reg_mode,
                                                                           double* __restrict__ part) {
  loss_sparse_pass(rowptr, colidx, XT, thetaT, m, f, lambda, reg_mode != kImpRegPlain, part,
                   [&](long long u, long long k, double s) {
                     const double r = val[k], w = wgt[k];
                     return w * (r - s) * (r - s) - (double)row_w0[u] * (double)col_w0[colidx[k]] * s * s;
                   });
}

// part[block] = lambda times the block's share of |X|_F^2 + |Y|_F^2 (the plain regulariser: the weighted Grams do not carry
// the unweighted norms); elements strided over the grid, so the sum does not depend on the device
__global__ __launch_bounds__(kLossThreads) void weighted_rank1_sqnorm_kernel(const float* __restrict__ XT, long long nx,
                                                                             const float* __restrict__ thetaT, long long ny,
                                                                             float lambda, double* __restrict__ part) {
  __shared__ double red[kLossThreads];
  const long long stride = (long long)gridDim.x * kLossThreads, e0 = (long long)blockIdx.x * kLossThreads + threadIdx.x;
  double acc = 0.0;
  for (long long e = e0; e < nx; e += stride) acc = fma((double)XT[e], (double)XT[e], acc);
  for (long long e = e0; e < ny; e += stride) acc = fma((double)thetaT[e], (double)thetaT[e], acc);
  const double t = loss_block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = (double)lambda * t;
}

// out = sum of the parts + <Gx, Gy>_F
__global__ __launch_bounds__(kLossThreads) void weighted_rank1_loss_final_kernel(const double* __restrict__ part, int nparts,
                                                                                 const double* __restrict__ Gx,
                                                                                 const double* __restrict__ Gy, int f,
                                                                                 double* __restrict__ out) {
  __shared__ double red[kLossThreads];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kLossThreads) acc += part[i];
  for (int e = threadIdx.x; e < f * f; e += kLossThreads) acc += Gx[e] * Gy[e];
  const double t = loss_block_sum(acc, red);
  if (threadIdx.x == 0) out[0] = t;
}

hipError_t launch_weighted_rank1_loss(const int* rowptr, const int* colidx, const float* val, const float* wgt, const float* XT,
                                      const float* thetaT, const float* row_w0, const float* col_w0, long m, long n, int f,
                                      float lambda, int reg_mode, const double* Gx, const double* Gy, double* part, double* out,
                                      hipStream_t stream) {
  hipError_t e = launch_kernel(weighted_rank1_loss_kernel, dim3(kImpLossBlocks), dim3(kLossThreads), 0, stream, rowptr, colidx,
                               val, wgt, XT, thetaT, row_w0, col_w0, (long long)m, f, lambda, reg_mode, part);
  if (e != hipSuccess) return e;
  int nparts = kImpLossBlocks;
  if (reg_mode == kImpRegPlain) {
    e = launch_kernel(weighted_rank1_sqnorm_kernel, dim3(kImpLossBlocks), dim3(kLossThreads), 0, stream, XT, (long long)m * f,
                      thetaT, (long long)n * f, lambda, part + kImpLossBlocks);
    if (e != hipSuccess) return e;
    nparts = 2 * kImpLossBlocks;
  }
  return launch_kernel(weighted_rank1_loss_final_kernel, dim3(1), dim3(kLossThreads), 0, stream, (const double*)part, nparts, Gx,
                       Gy, f, out);
}

}  // namespace cumf
