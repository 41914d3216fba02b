// als_free_core.h -- the device core of the matrix-free CGs: the explicit one (als_free.hip: A_u v = T_u^T (T_u v) + reg v),
// the implicit one (als_implicit_free.hip: A_u v = G v + T_u^T (w o (T_u v)) + reg v) and the two weighted ones (als_weighted.hip:
// A_u v = w0 G v + T_u^T ((w - w0) o (T_u v)) + reg v, and with rank-one weights a_u c_i on the unstored entries
// A_u v = a_u G_c v + T_u^T ((w - a_u c) o (T_u v)) + reg v).  T_u is the row's gathered block of factor rows.  The kernels of
// the three files are wrappers around
//   free_sparse_pass  one wave per SEGMENT of a row (at most kFreeSeg entries, cut at fixed offsets from the row's start): per
//                     block of N entries s = T v by the transposing wave reduction, then T^T s (with weights: T^T (w o s))
//                     accumulated in entry order, written as one f-vector partial per segment; the first pass of a
//                     half-iteration also writes the segment's part of b;
//   free_gram_rows    kFreeRows rows per workgroup: their vectors staged in LDS and G v of all of them on the matrix pipe, then
//                     free_row_update of each live row;
//   free_row_update   one wave on one live row: sums the segment partials in segment order, adds reg v (kGram: and the row's
//                     G v) and runs the CG scalar and vector updates of cumf_cg_solve_batched (exit when r.r < 1e-4, a done
//                     flag per row).
// Every sum runs in a fixed order.  No float atomics.
#ifndef CUMF_ALS_FREE_CORE_H_
#define CUMF_ALS_FREE_CORE_H_

#include <hip/hip_runtime.h>

#include "als_device.h"
#include "als_free.h"

namespace cumf {

constexpr int kFreeThreads = 256;  // four waves

// ---- the sparse pass: lane l holds features l + 64 q (q < Q = ceil(f / 64)) of every vector.
// first: v = x (the warm start) and the segment's part of b is written too; otherwise v = p.
// Where entry e takes its weight in T^T (w o s) and its coefficient in b from:
//   kFreeWeightNone   no weight, coefficient val;
//   kFreeWeightAlpha  the confidence weight w = wpar |val| (wpar = alpha), coefficient (val > 0 ? 1 + w : 0);
//   kFreeWeightArray  w = wgt[e] - wpar (wpar = w0, the weight of the unstored entries), coefficient wgt[e] val; wgt is
//                     indexed as val;
//   kFreeWeightRank1  w = fma(-own_w0[row], gather_w0[j], wgt[e]) (the unstored entries of row `row` and column j weigh
//                     own_w0[row] gather_w0[j]; wpar is not read), coefficient wgt[e] val.  own_w0 is indexed as the rows of
//                     the args (wave-uniform), gather_w0 as the rows of `gather`: one 4-byte gather by the column index the
//                     lane holds.  With gather_w0 = 1 the weight is wgt[e] - own_w0[row] rounded once: kFreeWeightArray's.
enum FreeWeight { kFreeWeightNone = 0, kFreeWeightAlpha = 1, kFreeWeightArray = 2, kFreeWeightRank1 = 3 };
template <int Q, FreeWeight kWeight>
__device__ __forceinline__ void free_sparse_pass(const FreeArgs a, int first, float wpar, const float* wgt = nullptr,
                                                 const float* own_w0 = nullptr, const float* gather_w0 = nullptr) {
  constexpr bool kWeighted = kWeight != kFreeWeightNone;
  constexpr int N = Q <= 4 ? 16 : 8;  // entries per block: N x Q <= 64 gathered values per lane (N = 32: SGPR spills)
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
    [[maybe_unused]] float aw = 0.f;  // kFreeWeightRank1: the row's factor of its unstored weights (uniform)
    if constexpr (kWeight == kFreeWeightRank1) aw = own_w0[row];
    for (int s = 0; s < len; s += 64) {
      const int cnt64 = len - s < 64 ? len - s : 64;
      const bool live = lane < cnt64;
      const int jl = live ? a.colidx[begin + s + lane] : 0;
      const float rl = live ? a.val[begin + s + lane] : 0.f;
      [[maybe_unused]] float wl = 0.f;  // weight of entry s + lane
      float cl = rl;                    // its coefficient in b
      if constexpr (kWeight == kFreeWeightAlpha) {
        wl = live ? wpar * fabsf(rl) : 0.f;
        cl = (live && rl > 0.f) ? 1.f + wl : 0.f;
      } else if constexpr (kWeight == kFreeWeightArray) {
        const float gl = live ? wgt[begin + s + lane] : 0.f;
        wl = live ? gl - wpar : 0.f;
        cl = gl * rl;
      } else if constexpr (kWeight == kFreeWeightRank1) {
        const float gl = live ? wgt[begin + s + lane] : 0.f;
        const float cj = live ? gather_w0[jl] : 0.f;
        wl = live ? fmaf(-aw, cj, gl) : 0.f;
        cl = gl * rl;
      }
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
        // lane L: s of entry b + (L mod N), kWeighted: times its weight
        float u;
        if constexpr (kWeighted)
          u = reduce_transposed<N>(P, lane) * __shfl(wl, b + (lane & (N - 1)));
        else
          u = reduce_transposed<N>(P, lane);
        static_for<N>([&](auto rc) {
          constexpr int r = decltype(rc)::value;
          if (r < cnt) {
            const float ur = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, u), r));
#pragma unroll
            for (int q = 0; q < Q; ++q) acc[q] = fmaf(T[r][q], ur, acc[q]);
            if (first) {
              const float cr = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, cl), b + r));
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

// ---- the row update of one wave on row `row` (not done) of n stored entries.  mode 0 (after the first sparse pass):
// r = b - A x, p = r, rs = r.r; mode 1: one CG step with A p.  last: the row is done after this pass.  kGram: gv[c] is
// feature c of the row's G v.
template <int Q, bool kGram>
__device__ __forceinline__ void free_row_update(const FreeArgs a, long long row, int n, float reg, const float* gv, int lane,
                                                int mode, int last) {
  const int f = a.f;
  auto dot = [&](const float(&u)[Q], const float(&w)[Q]) {
    float d = u[0] * w[0];
#pragma unroll
    for (int q = 1; q < Q; ++q) d = fmaf(u[q], w[q], d);
    return wave_sum_uniform(d);
  };
  const size_t o = (size_t)row * f;
  if (n == 0) {  // no stored entry: x = 0 (b = 0)
#pragma unroll
    for (int q = 0; q < Q; ++q)
      if (lane + 64 * q < f) a.x[o + lane + 64 * q] = 0.f;
    if (lane == 0) a.done[row] = 1;
    return;
  }
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
    if constexpr (kGram)
      ap[q] = c < f ? fmaf(reg, v[q], gv[c] + sp) : 0.f;
    else
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

// ---- the row pass with G v: kFreeRows rows per workgroup of kFreeThreads.  mode 0 (after the first sparse pass):
// r = b - A x, p = r, rs = r.r; mode 1: one CG step with A p.  last: the rows are done after this pass.  Args: FreeArgs
// extended by G (the f x f Gram of `gather`) and reg_mode (kFreeRegPlain: reg = lambda, else (float)n lambda).  kScale: what
// G v is multiplied by as it leaves the accumulators -- nothing, gscale (the weighted route's w0; at gscale = 1 the product
// is the factor itself, bit for bit) or row_scale[row] (the rank-one route's own_w0, indexed as the rows of the args; rows
// beyond the block's last read nothing).
enum FreeScale { kFreeScaleNone = 0, kFreeScaleScalar = 1, kFreeScaleRow = 2 };
template <int Q, FreeScale kScale, class Args>
__device__ __forceinline__ void free_gram_rows(const Args& a, float gscale, int mode, int last,
                                               const float* row_scale = nullptr) {
  constexpr int P = 64 * Q + 4;  // LDS pitch: the 16 rows one MFMA operand reads start 4 banks apart
  __shared__ float vs[kFreeRows * P];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int f = a.f, FT = (f + 15) / 16, FP = 16 * FT;
  const long long r0 = (long long)blockIdx.x * kFreeRows;
  const int nr = (int)(a.rows - r0 < kFreeRows ? a.rows - r0 : kFreeRows);
  if (!__syncthreads_or((int)threadIdx.x < nr && !a.done[r0 + threadIdx.x])) return;  // every row of the block is done
  const float* V = mode == 0 ? a.x : a.p;
  for (int e = threadIdx.x; e < kFreeRows * FP; e += kFreeThreads) {
    const int rr = e / FP, c = e - rr * FP;
    vs[rr * P + c] = (rr < nr && c < f) ? V[(size_t)(r0 + rr) * f + c] : 0.f;
  }
  __syncthreads();
  // G v of the block's rows: wave w takes the 16-column tiles J = w + 4 t of both 16-row tiles; v_mfma_f32_16x16x4_f32 with
  // A[i][k] = v_i[k] (LDS) and B[k][j] = G[k][16 J + j] (G symmetric, read from L2)
  f32x4 acc[Q][2];
#pragma unroll
  for (int t = 0; t < Q; ++t) acc[t][0] = acc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kk = 0; kk < FP / 4; ++kk) {
    const int k = 4 * kk + (lane >> 4);
    const float a0 = vs[(lane & 15) * P + k], a1 = vs[(16 + (lane & 15)) * P + k];
#pragma unroll
    for (int t = 0; t < Q; ++t) {
      const int J = wave + 4 * t;
      if (J < FT) {  // uniform
        const int c = 16 * J + (lane & 15);
        const float g = (k < f && c < f) ? a.G[(size_t)k * f + c] : 0.f;
        acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, g, acc[t][0], 0, 0, 0);
        acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, g, acc[t][1], 0, 0, 0);
      }
    }
  }
  __syncthreads();
  [[maybe_unused]] float rsc[2][4];  // kFreeScaleRow: the scales of the eight accumulator rows this lane holds
  if constexpr (kScale == kFreeScaleRow) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = 16 * h + 4 * (lane >> 4) + r;
        rsc[h][r] = rr < nr ? row_scale[r0 + rr] : 0.f;
      }
  }
#pragma unroll
  for (int t = 0; t < Q; ++t) {
    const int J = wave + 4 * t;
    if (J < FT) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float g = acc[t][h][r];
          if constexpr (kScale == kFreeScaleScalar) g = g * gscale;
          if constexpr (kScale == kFreeScaleRow) g = g * rsc[h][r];
          vs[(16 * h + 4 * (lane >> 4) + r) * P + 16 * J + (lane & 15)] = g;
        }
    }
  }
  __syncthreads();
  for (int rr = wave; rr < nr; rr += 4) {
    const long long row = r0 + rr;
    if (a.done[row]) continue;  // uniform
    const int n = a.row_len[row];
    const float reg = a.reg_mode == kFreeRegPlain ? a.lambda : (float)n * a.lambda;
    free_row_update<Q, true>(a, row, n, reg, vs + rr * P, lane, mode, last);
  }
}

// workgroups of `per_block` units over `work` units, at most `cap` (the sparse pass strides over the rest)
inline unsigned free_grid(long long work, long long per_block, long long cap) {
  const long long g = (work + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

}  // namespace cumf

#endif  // CUMF_ALS_FREE_CORE_H_
