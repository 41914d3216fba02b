// als_implicit_free.hip -- implicit-feedback ALS at any even 8 <= f <= 512: the operator-only ("matrix-free") CG of
// CUMF_SOLVER_CG_MATFREE (include/cumf_implicit_capi.h) and the Gram of tables wider than 128 features, plain
// (implicit_gram_wide_kernel) and with a weight per table row (weighted_gram_wide_kernel; include/cumf_weighted_capi.h).
//
// The CG never forms A_u.  Each step needs, for every live row u, A_u v = G v + T_u^T (w o (T_u v)) + reg_u v (T_u the
// row's gathered block of factor rows, w its confidence weights): the core of als_free_core.h with the weights and with G v.
//   implicit_free_sparse_kernel  one wave per segment of a row (free_sparse_pass); b = sum_{r>0} (1 + w) y;
//   implicit_free_row_kernel     kFreeRows rows per workgroup (free_gram_rows): their vectors staged in LDS, G v of all of
//                                them on v_mfma_f32_16x16x4_f32 (G streamed from L2 once per block, never once per row), then
//                                one wave per row (free_row_update).
// A row's result does not depend on which other rows share its workgroup or plan: the factors are bit-identical from run to
// run and for any x_batch / theta_batch.
#include <hip/hip_runtime.h>

#include "als_free_core.h"
#include "als_implicit.h"

namespace cumf {

constexpr int kGramGroup = 36;     // upper tiles per workgroup of the wide Gram: nine per wave, the budget of the FT = 8 kernel
constexpr int kGramStage = 32;     // table rows per LDS stage
constexpr int kGramPitch = 512 + 16;

// tile t of the upper triangle of an FT x FT grid of 16 x 16 tiles, row-major: (I, J), I <= J
__device__ inline void free_upper_tile(int t, int FT, int& I, int& J) {
  I = 0;
  while (t >= FT - I) {
    t -= FT - I;
    ++I;
  }
  J = I + t;
}

// ---- G = Y^T Y for 128 < f <= 512: workgroup (slab, group) accumulates the group's upper tiles over the slab's rows (the
// arithmetic of implicit_gram_partial_kernel) and writes them into the slab's FP x FP partial; implicit_gram_reduce_kernel
// sums the partials in slab order.
__global__ __launch_bounds__(kFreeThreads) void implicit_gram_wide_kernel(const float* __restrict__ Y, long long rows, int f,
                                                                         int slab, float* __restrict__ part) {
  constexpr int TPW = kGramGroup / 4;
  __shared__ float ys[kGramStage * kGramPitch];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int FT = (f + 15) / 16, FP = 16 * FT, NT = FT * (FT + 1) / 2;
  const int t0 = (int)blockIdx.y * kGramGroup + wave;
  int I[TPW], J[TPW];
  f32x4 acc[TPW];
#pragma unroll
  for (int q = 0; q < TPW; ++q) {
    I[q] = J[q] = 0;
    if (t0 + 4 * q < NT) free_upper_tile(t0 + 4 * q, FT, I[q], J[q]);
    acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const long long r0 = (long long)blockIdx.x * slab;
  const int n = (int)(rows - r0 < slab ? rows - r0 : slab);
  for (int s = 0; s < n; s += kGramStage) {
    const int cnt = n - s < kGramStage ? n - s : kGramStage;
    __syncthreads();
    for (int e = threadIdx.x; e < kGramStage * FP; e += kFreeThreads) {
      const int r = e / FP, c = e - r * FP;
      ys[r * kGramPitch + c] = (r < cnt && c < f) ? Y[(size_t)(r0 + s + r) * f + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kGramStage / 4; ++kk) {
      const float* yk = ys + (4 * kk + (lane >> 4)) * kGramPitch + (lane & 15);
#pragma unroll
      for (int q = 0; q < TPW; ++q)
        if (t0 + 4 * q < NT) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(yk[16 * I[q]], yk[16 * J[q]], acc[q], 0, 0, 0);
    }
  }
  float* out = part + (size_t)blockIdx.x * FP * FP;
#pragma unroll
  for (int q = 0; q < TPW; ++q) {
    if (t0 + 4 * q < NT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(16 * I[q] + 4 * (lane >> 4) + r) * FP + 16 * J[q] + (lane & 15)] = acc[q][r];
    }
  }
}

// ---- G = Y^T diag(row_w) Y for 128 < f <= 512 (include/cumf_weighted_capi.h): implicit_gram_wide_kernel with the A operand
// of table row k scaled by row_w[k] (staged in LDS beside the rows) -- the same slabs, stages, tiles and k order, so that at
// row_w = 1, where 1 y is y, the partials are its bits.  A kernel of its own, not a second instantiation of a shared body:
// moving any part of the kernel above into a function changes the code generated for it (tools/kernels_equal.py).
__global__ __launch_bounds__(kFreeThreads) void weighted_gram_wide_kernel(const float* __restrict__ Y,
                                                                         const float* __restrict__ row_w, long long rows, int f,
                                                                         int slab, float* __restrict__ part) {
  constexpr int TPW = kGramGroup / 4;
  __shared__ float ys[kGramStage * kGramPitch];
  __shared__ float sw[kGramStage];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int FT = (f + 15) / 16, FP = 16 * FT, NT = FT * (FT + 1) / 2;
  const int t0 = (int)blockIdx.y * kGramGroup + wave;
  int I[TPW], J[TPW];
  f32x4 acc[TPW];
#pragma unroll
  for (int q = 0; q < TPW; ++q) {
    I[q] = J[q] = 0;
    if (t0 + 4 * q < NT) free_upper_tile(t0 + 4 * q, FT, I[q], J[q]);
    acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const long long r0 = (long long)blockIdx.x * slab;
  const int n = (int)(rows - r0 < slab ? rows - r0 : slab);
  for (int s = 0; s < n; s += kGramStage) {
    const int cnt = n - s < kGramStage ? n - s : kGramStage;
    __syncthreads();
    for (int e = threadIdx.x; e < kGramStage * FP; e += kFreeThreads) {
      const int r = e / FP, c = e - r * FP;
      ys[r * kGramPitch + c] = (r < cnt && c < f) ? Y[(size_t)(r0 + s + r) * f + c] : 0.f;
    }
    if ((int)threadIdx.x < kGramStage) sw[threadIdx.x] = (int)threadIdx.x < cnt ? row_w[r0 + s + threadIdx.x] : 0.f;
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kGramStage / 4; ++kk) {
      const float* yk = ys + (4 * kk + (lane >> 4)) * kGramPitch + (lane & 15);
      const float wk = sw[4 * kk + (lane >> 4)];
#pragma unroll
      for (int q = 0; q < TPW; ++q)
        if (t0 + 4 * q < NT) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(wk * yk[16 * I[q]], yk[16 * J[q]], acc[q], 0, 0, 0);
    }
  }
  float* out = part + (size_t)blockIdx.x * FP * FP;
#pragma unroll
  for (int q = 0; q < TPW; ++q) {
    if (t0 + 4 * q < NT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(16 * I[q] + 4 * (lane >> 4) + r) * FP + 16 * J[q] + (lane & 15)] = acc[q][r];
    }
  }
}

// row_w: nullptr for G = Y^T Y, else the weight of each table row
hipError_t launch_implicit_gram_wide(const float* Y, const float* row_w, long rows, int f, float* part, hipStream_t stream) {
  const int FT = (f + 15) / 16, NT = FT * (FT + 1) / 2;
  const long slab = implicit_gram_slab(f);
  const unsigned nslab = (unsigned)((rows + slab - 1) / slab), groups = (unsigned)((NT + kGramGroup - 1) / kGramGroup);
  if (row_w)
    return launch_kernel(weighted_gram_wide_kernel, dim3(nslab, groups), dim3(kFreeThreads), 0, stream, Y, row_w,
                         (long long)rows, f, (int)slab, part);
  return launch_kernel(implicit_gram_wide_kernel, dim3(nslab, groups), dim3(kFreeThreads), 0, stream, Y, (long long)rows, f,
                       (int)slab, part);
}

template <int Q>
__global__ __launch_bounds__(kFreeThreads) void implicit_free_sparse_kernel(const ImplicitFreeArgs a, int first) {
  free_sparse_pass<Q, kFreeWeightAlpha>(a, first, a.alpha);
}

// ---- the row pass: kFreeRows rows per workgroup.  mode 0 (after the first sparse pass): r = b - A x, p = r, rs = r.r;
// mode 1: one CG step with A p.  last: the rows are done after this pass.
template <int Q>
__global__ __launch_bounds__(kFreeThreads) void implicit_free_row_kernel(const ImplicitFreeArgs a, int mode, int last) {
  free_gram_rows<Q, kFreeScaleNone>(a, 1.f, mode, last);
}

hipError_t launch_implicit_free_pass(const ImplicitFreeArgs& a, int step, int cg_iters, hipStream_t stream) {
  const int Q = (a.f + 63) / 64;
  const int first = step == 0, last = step >= cg_iters;
  return with_nb<1, 8>(Q, [&](auto qc) {
    constexpr int QC = decltype(qc)::value;
    hipError_t e = hipSuccess;
    if (a.nseg > 0)
      e = launch_kernel(implicit_free_sparse_kernel<QC>, dim3(free_grid(a.nseg, 4, 16384)), dim3(kFreeThreads), 0, stream, a,
                        first);
    if (e != hipSuccess) return e;
    return launch_item_kernel(implicit_free_row_kernel<QC>, dim3(free_grid(a.rows, kFreeRows, 1ll << 30)), dim3(kFreeThreads),
                              0, stream, a, first ? 0 : 1, last);
  });
}

}  // namespace cumf
