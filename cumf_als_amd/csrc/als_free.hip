// als_free.hip -- explicit-feedback ALS at any even 8 <= f <= 512 without a Gram matrix: the operator-only ("matrix-free")
// CG of include/cumf_free_capi.h.  The CG never forms A_u.  Each step needs, for every live row u,
// A_u v = T_u^T (T_u v) + reg_u v (T_u the row's gathered block of factor rows): the core of als_free_core.h without weights
// and without G v, so no matrix-pipe pass and no LDS.
//   free_sparse_kernel  one wave per segment of a row (free_sparse_pass);
//   free_row_kernel     one wave per row (free_row_update).
// A row's result depends on its own entries, warm start, f, lambda and cg_iters only: the factors are bit-identical from run
// to run and for any x_batch / theta_batch / chunk.
#include <hip/hip_runtime.h>

#include "als_free_core.h"

namespace cumf {

template <int Q>
__global__ __launch_bounds__(kFreeThreads) void free_sparse_kernel(const FreeArgs a, int first) {
  free_sparse_pass<Q, kFreeWeightNone>(a, first, 0.f);
}

template <int Q>
__global__ __launch_bounds__(kFreeThreads) void free_row_kernel(const FreeArgs a, int mode, int last) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long row = (long long)blockIdx.x * 4 + wave;
  if (row >= a.rows || a.done[row]) return;  // uniform
  const int n = a.row_len[row];
  free_row_update<Q, false>(a, row, n, (float)n * a.lambda, nullptr, lane, mode, last);
}

hipError_t launch_free_pass(const FreeArgs& a, int step, int cg_iters, hipStream_t stream) {
  const int Q = (a.f + 63) / 64;
  const int first = step == 0, last = step >= cg_iters;
  if (a.rows <= 0 || a.rows > (1ll << 32)) return a.rows ? hipErrorInvalidValue : hipSuccess;  // one wave per row, no stride
  return with_nb<1, 8>(Q, [&](auto qc) {
    constexpr int QC = decltype(qc)::value;
    hipError_t e = hipSuccess;
    if (a.nseg > 0)
      e = launch_kernel(free_sparse_kernel<QC>, dim3(free_grid(a.nseg, 4, 16384)), dim3(kFreeThreads), 0, stream, a, first);
    if (e != hipSuccess) return e;
    return launch_item_kernel(free_row_kernel<QC>, dim3(free_grid(a.rows, 4, 1ll << 30)), dim3(kFreeThreads), 0, stream, a,
                              first ? 0 : 1, last);
  });
}

}  // namespace cumf
