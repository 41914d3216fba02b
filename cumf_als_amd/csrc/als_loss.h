// als_loss.h -- what the fp64 objectives of the implicit model (als_implicit.hip) and of the weighted one (als_weighted.hip)
// share on the device: the fixed-order workgroup sum and the pass over the stored entries.  Both objectives are
//   sum over the stored entries of term(entry, s) (+ lambda (|x_u|^2 + |y_i|^2) per entry when reg is lambda n) + a Gram term,
// s = x_u . y_i; they differ in the per-entry term and in the Gram term of their final kernels.
#ifndef CUMF_ALS_LOSS_H_
#define CUMF_ALS_LOSS_H_

#include <hip/hip_runtime.h>

#include <type_traits>

namespace cumf {

constexpr int kLossThreads = 256;  // four waves

// fixed-order sum of the workgroup's values (thread 0 returns it); red: kLossThreads doubles of LDS
__device__ __forceinline__ double loss_block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kLossThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// part[block] = sum over its rows' stored entries k of term(k, s) (+ lambda (|x_u|^2 + |y_i|^2) when reg_per_entry: sum_u
// lambda n_u |x_u|^2 = sum over the stored entries of lambda |x_u|^2, the same for Y).  One wave per row, rows strided over
// the grid, so the sum does not depend on the device.  A term that takes three arguments gets the row too: term(u, k, s).
template <class Term>
__device__ __forceinline__ void loss_sparse_pass(const int* __restrict__ rowptr, const int* __restrict__ colidx,
                                                 const float* __restrict__ XT, const float* __restrict__ thetaT, long long m,
                                                 int f, float lambda, bool reg_per_entry, double* __restrict__ part,
                                                 Term term) {
  __shared__ double red[kLossThreads];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double lam = lambda;
  double acc = 0.0;
  for (long long u = (long long)blockIdx.x * 4 + wave; u < m; u += (long long)gridDim.x * 4) {
    const float* x = XT + (size_t)u * f;
    for (long long k = rowptr[u] + lane; k < rowptr[u + 1]; k += 64) {
      const float* y = thetaT + (size_t)colidx[k] * f;
      double s = 0.0, xx = 0.0, yy = 0.0;
      for (int c = 0; c < f; ++c) {
        const double xc = x[c], yc = y[c];
        s = fma(xc, yc, s);
        xx = fma(xc, xc, xx);
        yy = fma(yc, yc, yy);
      }
      if constexpr (std::is_invocable_v<Term, long long, long long, double>)
        acc += term(u, k, s);
      else
        acc += term(k, s);
      if (reg_per_entry) acc += lam * (xx + yy);
    }
  }
  const double t = loss_block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

}  // namespace cumf

#endif  // CUMF_ALS_LOSS_H_
