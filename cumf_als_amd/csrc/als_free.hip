// als_free.hip -- explicit-feedback ALS at any even 8 <= f <= 512 without a Gram matrix: the operator-only ("matrix-free")
// CG of include/cumf_free_capi.h.  The shape of als_implicit_free.hip without its G v: no matrix-pipe pass, no LDS.
//
// The CG never forms A_u.  Each step needs, for every live row u, A_u v = T_u^T (T_u v) + reg_u v (T_u the row's gathered
// block of factor rows):
//   free_sparse_kernel  one wave per SEGMENT of a row (at most kFreeSeg entries, cut at fixed offsets from the row's start):
//                       per block of N entries s = T v by the transposing wave reduction, then T^T s accumulated in entry
//                       order, written as one f-vector partial per segment; the first pass of a half-iteration also writes
//                       the segment's part of b = T^T r;
//   free_row_kernel     one wave per row: sums the segment partials in segment order, adds reg v and runs the CG scalar and
//                       vector updates of cumf_cg_solve_batched (exit when r.r < 1e-4, a done flag per row).
// Every sum runs in a fixed order and a row's result depends on its own entries, warm start, f, lambda and cg_iters only:
// the factors are bit-identical from run to run and for any x_batch / theta_batch / chunk.  No float atomics.
#include <hip/hip_runtime.h>

#include "als_device.h"
#include "als_free.h"

namespace cumf {

constexpr int kFreeThreads = 256;  // four waves

// ---- the sparse pass: one wave per segment; lane l holds features l + 64 q (q < Q = ceil(f / 64)) of every vector.
// first: v = x (the warm start) and the segment's part of b is written too; otherwise v = p.
template <int Q>
__global__ __launch_bounds__(kFreeThreads) void free_sparse_kernel(const FreeArgs a, int first) {
  constexpr int N = Q <= 4 ? 16 : 8;  // entries per block: N x Q <= 64 gathered values per lane
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int f = a.f;
  const float* V = first ? a.x : a.p;
  for (long long sg = (long long)blockIdx.x * 4 + wave; sg < a.nseg; sg += (long long)gridDim.x * 4) {
    const int row = a.seg_row[sg];
    if (a.done[row]) continue;  // uniform
    const long long begin = a.seg_begin[sg];
    const int len = a.seg_len[sg];
    float v[Q], acc[Q], bacc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int c = lane + 64 * q;
      v[q] = c < f ? V[(size_t)row * f + c] : 0.f;
      acc[q] = bacc[q] = 0.f;
    }
    for (int s = 0; s < len; s += 64) {
      const int cnt64 = len - s < 64 ? len - s : 64;
      const bool live = lane < cnt64;
      const int jl = live ? a.colidx[begin + s + lane] : 0;
      const float rl = live ? a.val[begin + s + lane] : 0.f;  // rating of entry s + lane: its coefficient in b
      for (int b = 0; b < cnt64; b += N) {
        const int cnt = cnt64 - b < N ? cnt64 - b : N;  // uniform
        float T[N][Q];
        static_for<N>([&](auto rc) {
          constexpr int r = decltype(rc)::value;
          if (r < cnt) {
            const int j = __builtin_amdgcn_readlane(jl, b + r);
            const float* y = a.gather + (size_t)j * f;
#pragma unroll
            for (int q = 0; q < Q; ++q) T[r][q] = lane + 64 * q < f ? y[lane + 64 * q] : 0.f;
          } else {
#pragma unroll
            for (int q = 0; q < Q; ++q) T[r][q] = 0.f;
          }
        });
        float P[N];
        static_for<N>([&](auto rc) {
          constexpr int r = decltype(rc)::value;
          float d = T[r][0] * v[0];
#pragma unroll
          for (int q = 1; q < Q; ++q) d = fmaf(T[r][q], v[q], d);
          P[r] = d;
        });
        const float u = reduce_transposed<N>(P, lane);  // lane L: s of entry b + (L mod N)
        static_for<N>([&](auto rc) {
          constexpr int r = decltype(rc)::value;
          if (r < cnt) {
            const float ur = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, u), r));
#pragma unroll
            for (int q = 0; q < Q; ++q) acc[q] = fmaf(T[r][q], ur, acc[q]);
            if (first) {
              const float cr = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, rl), b + r));
#pragma unroll
              for (int q = 0; q < Q; ++q) bacc[q] = fmaf(T[r][q], cr, bacc[q]);
            }
          }
        });
      }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int c = lane + 64 * q;
      if (c < f) {
        a.part[(size_t)sg * f + c] = acc[q];
        if (first) a.bpart[(size_t)sg * f + c] = bacc[q];
      }
    }
  }
}

// ---- the row pass: one wave per row.  mode 0 (after the first sparse pass): r = b - A x, p = r, rs = r.r; mode 1: one CG
// step with A p.  last: the rows are done after this pass.
template <int Q>
__global__ __launch_bounds__(kFreeThreads) void free_row_kernel(const FreeArgs a, int mode, int last) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int f = a.f;
  const long long row = (long long)blockIdx.x * 4 + wave;
  if (row >= a.rows || a.done[row]) return;  // uniform
  auto dot = [&](const float(&u)[Q], const float(&w)[Q]) {
    float d = u[0] * w[0];
#pragma unroll
    for (int q = 1; q < Q; ++q) d = fmaf(u[q], w[q], d);
    return wave_sum_uniform(d);
  };
  const int n = a.row_len[row];
  const size_t o = (size_t)row * f;
  if (n == 0) {  // no stored entry: x = 0 (b = 0)
#pragma unroll
    for (int q = 0; q < Q; ++q)
      if (lane + 64 * q < f) a.x[o + lane + 64 * q] = 0.f;
    if (lane == 0) a.done[row] = 1;
    return;
  }
  const float reg = (float)n * a.lambda;
  const int seg0 = a.row_seg0[row], ns = a.row_nseg[row];
  const float* V = mode == 0 ? a.x : a.p;
  float v[Q], ap[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int c = lane + 64 * q;
    v[q] = c < f ? V[o + c] : 0.f;
    float sp = 0.f;
    if (c < f)
      for (int k = 0; k < ns; ++k) sp += a.part[(size_t)(seg0 + k) * f + c];
    ap[q] = c < f ? fmaf(reg, v[q], sp) : 0.f;
  }
  if (mode == 0) {
    float r[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int c = lane + 64 * q;
      float b = 0.f;
      if (c < f)
        for (int k = 0; k < ns; ++k) b += a.bpart[(size_t)(seg0 + k) * f + c];
      r[q] = b - ap[q];
      if (c < f) a.r[o + c] = r[q], a.p[o + c] = r[q];
    }
    const float rs = dot(r, r);
    if (lane == 0) {
      a.rs[row] = rs;
      if (last) a.done[row] = 1;
    }
  } else {
    const float rsold = a.rs[row];
    const float alpha = rsold / dot(v, ap);
    float r[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int c = lane + 64 * q;
      r[q] = c < f ? fmaf(-alpha, ap[q], a.r[o + c]) : 0.f;
      if (c < f) a.x[o + c] = fmaf(alpha, v[q], a.x[o + c]), a.r[o + c] = r[q];
    }
    const float rsnew = dot(r, r);
    if ((double)rsnew < 1e-4 || last) {  // CG_ERROR (cg.cu:31,195), or the last step
      if (lane == 0) a.done[row] = 1;
    } else {
      const float beta = rsnew / rsold;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int c = lane + 64 * q;
        if (c < f) a.p[o + c] = fmaf(beta, v[q], r[q]);
      }
      if (lane == 0) a.rs[row] = rsnew;
    }
  }
}

// workgroups of four waves over `work` waves, at most `cap` (the sparse pass strides over the rest)
static unsigned free_grid(long long work, long long cap) {
  const long long g = (work + 3) / 4;
  return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

hipError_t launch_free_pass(const FreeArgs& a, int step, int cg_iters, hipStream_t stream) {
  const int Q = (a.f + 63) / 64;
  const int first = step == 0, last = step >= cg_iters;
  if (a.rows <= 0 || a.rows > (1ll << 32)) return a.rows ? hipErrorInvalidValue : hipSuccess;  // one wave per row, no stride
  return with_nb<1, 8>(Q, [&](auto qc) {
    constexpr int QC = decltype(qc)::value;
    hipError_t e = hipSuccess;
    if (a.nseg > 0)
      e = launch_kernel(free_sparse_kernel<QC>, dim3(free_grid(a.nseg, 16384)), dim3(kFreeThreads), 0, stream, a, first);
    if (e != hipSuccess) return e;
    return launch_item_kernel(free_row_kernel<QC>, dim3(free_grid(a.rows, 1ll << 30)), dim3(kFreeThreads), 0, stream, a,
                              first ? 0 : 1, last);
  });
}

}  // namespace cumf
