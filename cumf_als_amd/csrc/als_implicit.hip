// als_implicit.hip -- the kernels of implicit-feedback ALS (Hu, Koren, Volinsky 2008; include/cumf_implicit_capi.h).
//
// A stored entry (u, i, r) has the weight w = alpha |r| and the preference p = (r > 0).  One side's systems are
//   A_u = G + sum_i w_ui y_i y_i^T + reg_u I,   b_u = sum_{r > 0} (1 + w_ui) y_i,   G = Y^T Y over the whole table.
// Five pieces, all on exact fp32 arithmetic with fixed reduction orders (bit-identical from run to run, no float atomics):
//   implicit_gram_partial_kernel   G of a table: one workgroup per slab of kImpGramSlab rows accumulates the upper 16 x 16 tiles
//                                  of its slab on v_mfma_f32_16x16x4_f32 and writes them; implicit_gram_reduce_kernel sums the
//                                  slab partials in slab order in fp64 and writes both triangles (exactly symmetric);
//   implicit_hermitian_kernel      one workgroup per plan item (a whole row, or one chunk of a long row): the weighted sum
//                                  sum w y y^T on the same MFMA (the A operand scaled by w), b on the VALU; a whole row writes
//                                  G + sum + reg I, a chunk its raw partial, which implicit_slot_reduce_kernel sums in chunk
//                                  order (fp64) for the row -- the partial-slot scheme of the explicit path;
//   ... in the packed output mode   the same item kernel with another epilogue (implicit_hermitian_kernel<kImpPacked + FT>):
//                                  the PARTIAL system a rank contributes to a multi-GPU sum -- no G, packed upper triangle,
//                                  lambda n on the diagonal in weighted mode; implicit_slot_reduce_packed_kernel likewise;
//                                  implicit_finish_kernel adds G (and lambda in plain mode) to the summed partials;
//   implicit_short_cg_kernel       rows of at most kShortRow entries: the CG of als_short.hip without forming A_u,
//                                  A p = G p + T^T (w o (T p)) + reg p, G shared by the waves of a workgroup in LDS;
//   implicit_loss_*                the objective from the stored entries and two fp64 Grams.
//
// Compiled twice (Makefile): as als_implicit_kernels.o, everything but the packed output mode, and with
// -DCUMF_IMPLICIT_PART=1 as als_implicit_partial.o, the packed output mode alone -- the item kernel's second set of
// instantiations, its slot reduce and the finish kernel.  An object of their own keeps the code generated for the first
// set exactly what it was before the second existed (tools/kernels_equal.py).  For the same reason a third time, with
// -DCUMF_IMPLICIT_PART=2 as als_implicit_wgram.o: weighted_gram_partial_kernel alone, the Gram with a weight per table row
// (G = Y^T diag(w) Y; include/cumf_weighted_capi.h), on the stage load and the weighted stage product of the item kernel.
#include <hip/hip_runtime.h>

#include "als_device.h"
#include "als_implicit.h"
#include "als_loss.h"

#ifndef CUMF_IMPLICIT_PART
#define CUMF_IMPLICIT_PART 0
#endif

namespace cumf {

// (no anonymous namespace: cumf_last_kernel_name reports the kernels as cumf::implicit_*; every name here is prefixed)
constexpr int kImpThreads = 256;  // four waves
static_assert(kImpThreads == kLossThreads, "the loss kernels run the workgroup sum of als_loss.h");
constexpr int kImpStage = 32;     // gathered rows per LDS stage

// LDS pitch of a stage of FP columns: the four rows one MFMA operand reads start 16 banks apart
__host__ __device__ constexpr int implicit_stage_pitch(int FP) { return ((FP + 63) / 64) * 64 + 16; }

// tile t of the upper triangle of an FT x FT grid of 16 x 16 tiles, row-major: (I, J), I <= J
__device__ inline void implicit_upper_tile(int t, int FT, int& I, int& J) {
  I = 0;
  while (t >= FT - I) {
    t -= FT - I;
    ++I;
  }
  J = I + t;
}

// The upper tiles of an FT x FT grid, TPW per wave (wave w takes tiles w, w + 4, ...): their block coordinates.
template <int FT>
struct ImplicitTiles {
  static constexpr int NT = FT * (FT + 1) / 2, TPW = (NT + 3) / 4;
  int I[TPW], J[TPW];
  __device__ explicit ImplicitTiles(int wave) {
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
      I[q] = J[q] = 0;
      if (wave + 4 * q < NT) implicit_upper_tile(wave + 4 * q, FT, I[q], J[q]);
    }
  }
};

// rows [0, cnt) of a stage into LDS (zeros beyond cnt and beyond f): src(r) is the r-th row of f floats
template <int FP, typename Src>
__device__ __forceinline__ void implicit_load_stage(float* ys, int cnt, int f, Src&& src) {
  constexpr int P = implicit_stage_pitch(FP);
  for (int e = threadIdx.x; e < kImpStage * FP; e += kImpThreads) {
    const int r = e / FP, c = e - r * FP;
    ys[r * P + c] = (r < cnt && c < f) ? src(r)[c] : 0.f;
  }
}

// acc[q] += sum over the stage's 32 rows k of (w_k y_k[16 I + i]) y_k[16 J + j] (tile q of this wave; w = 1 unweighted).
// v_mfma_f32_16x16x4_f32: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; the result is the k-ordered
// fp32 fma chain.
template <int FT, bool WEIGHTED>
__device__ __forceinline__ void implicit_stage_tiles(const float* ys, const float* sw, const ImplicitTiles<FT>& T,
                                            f32x4 (&acc)[ImplicitTiles<FT>::TPW], int wave, int lane) {
  constexpr int P = implicit_stage_pitch(16 * FT), TPW = ImplicitTiles<FT>::TPW, NT = ImplicitTiles<FT>::NT;
#pragma unroll
  for (int kk = 0; kk < kImpStage / 4; ++kk) {
    const int k = 4 * kk + (lane >> 4);
    const float* yk = ys + k * P + (lane & 15);
    const float wk = WEIGHTED ? sw[k] : 1.f;
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
      if (wave + 4 * q < NT) {  // wave-uniform
        const float av = WEIGHTED ? wk * yk[16 * T.I[q]] : yk[16 * T.I[q]];
        acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, yk[16 * T.J[q]], acc[q], 0, 0, 0);
      }
    }
  }
}

#if CUMF_IMPLICIT_PART == 0
// ---- 1. G = Y^T Y

template <int FT>
__global__ __launch_bounds__(kImpThreads) void implicit_gram_partial_kernel(const float* __restrict__ Y, long long rows, int f,
                                                                            float* __restrict__ part) {
  constexpr int FP = 16 * FT, TPW = ImplicitTiles<FT>::TPW, NT = ImplicitTiles<FT>::NT;
  __shared__ float ys[kImpStage * implicit_stage_pitch(FP)];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const ImplicitTiles<FT> T(wave);
  f32x4 acc[TPW];
#pragma unroll
  for (int q = 0; q < TPW; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  const long long r0 = (long long)blockIdx.x * kImpGramSlab;
  const int n = (int)(rows - r0 < kImpGramSlab ? rows - r0 : kImpGramSlab);
  for (int s = 0; s < n; s += kImpStage) {
    const int cnt = n - s < kImpStage ? n - s : kImpStage;
    __syncthreads();
    implicit_load_stage<FP>(ys, cnt, f, [&](int r) { return Y + (size_t)(r0 + s + r) * f; });
    __syncthreads();
    implicit_stage_tiles<FT, false>(ys, nullptr, T, acc, wave, lane);
  }
  // the upper tiles of the slab's FP x FP partial (C/D: column lane & 15, row 4 (lane >> 4) + reg)
  float* out = part + (size_t)blockIdx.x * FP * FP;
#pragma unroll
  for (int q = 0; q < TPW; ++q) {
    if (wave + 4 * q < NT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(16 * T.I[q] + 4 * (lane >> 4) + r) * FP + 16 * T.J[q] + (lane & 15)] = acc[q][r];
    }
  }
}

// Element (i, j) of G is entry (min, max) of the upper partials summed in slab order; a diagonal tile holds both (i, j) and
// (j, i) with the same bits (the same products in the same order), so the result is exactly symmetric.
__global__ __launch_bounds__(kImpThreads) void implicit_gram_reduce_kernel(const float* __restrict__ part, int nslab, int f,
                                                                           int FP, float* __restrict__ G,
                                                                           double* __restrict__ G64) {
  const int e = blockIdx.x * kImpThreads + threadIdx.x;
  if (e >= f * f) return;
  const int i = e / f, j = e - i * f;
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  double s = 0.0;
  for (int k = 0; k < nslab; ++k) s += (double)part[(size_t)k * FP * FP + lo * FP + hi];
  if (G) G[e] = (float)s;
  if (G64) G64[e] = s;
}

#endif  // CUMF_IMPLICIT_PART == 0

// ---- 2. materialised systems

// element (i, j), i <= j, of a packed upper triangle of order f (row-major: the layout of cumf_get_hermitian_packed)
__host__ __device__ constexpr int implicit_packed_index(int i, int j, int f) { return i * f - i * (i - 1) / 2 + (j - i); }

// MODE = FT: the systems of cumf_get_hermitian_implicit.  MODE = kImpPacked + FT, the packed output mode: the partial system
// of cumf_get_hermitian_implicit_partial -- a.tt is the batch of packed upper triangles, G is not read, and the diagonal of a
// whole row gets lambda n (weighted mode) or nothing (plain mode).  A chunk writes its raw partial either way.  (One template
// argument, so that the instantiations of the first mode keep their symbols.)
constexpr int kImpPacked = 16;
template <int MODE>
__global__ __launch_bounds__(kImpThreads) void implicit_hermitian_kernel(const ImplicitArgs a) {
  constexpr bool PACKED = MODE >= kImpPacked;
  constexpr int FT = MODE % kImpPacked;
  constexpr int FP = 16 * FT, P = implicit_stage_pitch(FP), TPW = ImplicitTiles<FT>::TPW, NT = ImplicitTiles<FT>::NT;
  __shared__ float ys[kImpStage * P];
  __shared__ float sw[kImpStage], sc[kImpStage];
  __shared__ int sj[kImpStage];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int item = blockIdx.x;
  const int f = a.f;
  const long long begin = a.item_begin[item];
  const int len = a.item_len[item], slot = a.item_slot[item];
  const ImplicitTiles<FT> T(wave);
  f32x4 acc[TPW];
#pragma unroll
  for (int q = 0; q < TPW; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bacc = 0.f;  // b of feature threadIdx.x (threads below f)
  for (int s = 0; s < len; s += kImpStage) {
    const int cnt = len - s < kImpStage ? len - s : kImpStage;
    __syncthreads();
    if (threadIdx.x < kImpStage) {
      const int t = threadIdx.x;
      const bool live = t < cnt;
      const float r = live ? a.val[begin + s + t] : 0.f;
      const float w = a.alpha * fabsf(r);
      sj[t] = live ? a.colidx[begin + s + t] : 0;
      sw[t] = w;
      sc[t] = r > 0.f ? 1.f + w : 0.f;
    }
    __syncthreads();
    implicit_load_stage<FP>(ys, cnt, f, [&](int r) { return a.gather + (size_t)sj[r] * f; });
    __syncthreads();
    implicit_stage_tiles<FT, true>(ys, sw, T, acc, wave, lane);
    if ((int)threadIdx.x < f)
      for (int r = 0; r < cnt; ++r) bacc = fmaf(sc[r], ys[r * P + threadIdx.x], bacc);
  }
  const size_t ff = (size_t)f * f;
  float *out, *rhs;
  bool whole = slot < 0;
  float reg = 0.f;
  if (whole) {
    const long long dst = a.item_dst ? a.item_dst[item] : a.item_row[item] - a.row_begin;
    out = a.tt + (size_t)dst * (PACKED ? (size_t)f * (f + 1) / 2 : ff);
    rhs = a.rhs ? a.rhs + (size_t)dst * f : nullptr;
    if constexpr (PACKED)
      reg = a.reg_mode == kImpRegPlain ? 0.f : a.lambda * (float)a.item_rowlen[item];
    else
      reg = a.reg_mode == kImpRegPlain ? a.lambda : a.lambda * (float)a.item_rowlen[item];
  } else {  // raw partial of one chunk: f x f + f floats per slot
    out = a.slots + (size_t)slot * (ff + f);
    rhs = out + ff;
  }
#pragma unroll
  for (int q = 0; q < TPW; ++q) {
    if (wave + 4 * q < NT) {
      const int gj = 16 * T.J[q] + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = 16 * T.I[q] + 4 * (lane >> 4) + r;
        if (gi < f && gj < f) {
          float v = acc[q][r];
          if constexpr (PACKED) {
            if (whole) {  // the upper triangle only (a diagonal tile holds both halves)
              if (gi == gj) v += reg;
              if (gi <= gj) out[implicit_packed_index(gi, gj, f)] = v;
              continue;
            }
          } else if (whole) {
            v = a.G[gi * f + gj] + v;
            if (gi == gj) v += reg;
          }
          out[(size_t)gi * f + gj] = v;
          if (T.I[q] != T.J[q]) out[(size_t)gj * f + gi] = v;  // the lower triangle mirrors the upper one
        }
      }
    }
  }
  if (rhs && (int)threadIdx.x < f) rhs[threadIdx.x] = bacc;
}

#if CUMF_IMPLICIT_PART == 0
// rows cut into chunks: G + (the chunk partials summed in chunk order, fp64) + reg I
__global__ __launch_bounds__(kImpThreads) void implicit_slot_reduce_kernel(const ImplicitArgs a) {
  const int m = blockIdx.x, f = a.f;
  const int slot0 = a.mrow_slot0[m], ns = a.mrow_nslots[m];
  const long long dst = a.mrow_dst ? a.mrow_dst[m] : a.mrow_row[m] - a.row_begin;
  const double reg = a.reg_mode == kImpRegPlain ? (double)a.lambda : (double)(a.lambda * (float)a.mrow_rowlen[m]);
  const int ff = f * f;
  for (int e = threadIdx.x; e < ff + f; e += kImpThreads) {
    double s = 0.0;
    for (int k = 0; k < ns; ++k) s += (double)a.slots[(size_t)(slot0 + k) * (ff + f) + e];
    if (e < ff) {
      const int i = e / f;
      a.tt[(size_t)dst * ff + e] = (float)((double)a.G[e] + s + (i == e - i * f ? reg : 0.0));
    } else if (a.rhs) {
      a.rhs[(size_t)dst * f + (e - ff)] = (float)s;
    }
  }
}

#elif CUMF_IMPLICIT_PART == 1
// the packed output mode of the slot reduce: the upper triangle of the chunk partials summed in chunk order (fp64), with
// lambda n on the diagonal in weighted mode; G is not read
__global__ __launch_bounds__(kImpThreads) void implicit_slot_reduce_packed_kernel(const ImplicitArgs a) {
  const int m = blockIdx.x, f = a.f;
  const int slot0 = a.mrow_slot0[m], ns = a.mrow_nslots[m];
  const long long dst = a.mrow_dst ? a.mrow_dst[m] : a.mrow_row[m] - a.row_begin;
  const double reg = a.reg_mode == kImpRegPlain ? 0.0 : (double)(a.lambda * (float)a.mrow_rowlen[m]);
  const int ff = f * f;
  for (int e = threadIdx.x; e < ff + f; e += kImpThreads) {
    const int i = e / f, j = e - i * f;
    if (e < ff && i > j) continue;  // below the diagonal
    double s = 0.0;
    for (int k = 0; k < ns; ++k) s += (double)a.slots[(size_t)(slot0 + k) * (ff + f) + e];
    if (e < ff)
      a.tt[(size_t)dst * (f * (f + 1) / 2) + implicit_packed_index(i, j, f)] = (float)(s + (i == j ? reg : 0.0));
    else if (a.rhs)
      a.rhs[(size_t)dst * f + (e - ff)] = (float)s;
  }
}

// tt[b] = (the packed upper triangle b, mirrored) + G, then + reg_add on the diagonal: two fp32 additions in this order
__global__ __launch_bounds__(kImpThreads) void implicit_finish_kernel(const float* __restrict__ packed,
                                                                      const float* __restrict__ G, float reg_add,
                                                                      float* __restrict__ tt, long long batch, int f) {
  const int ff = f * f, pk = f * (f + 1) / 2;
  const long long total = batch * ff;
  for (long long e = (long long)blockIdx.x * kImpThreads + threadIdx.x; e < total; e += (long long)gridDim.x * kImpThreads) {
    const long long b = e / ff;
    const int r = (int)(e - b * ff), i = r / f, j = r - i * f;
    float v = packed[(size_t)b * pk + (i < j ? implicit_packed_index(i, j, f) : implicit_packed_index(j, i, f))] + G[r];
    if (i == j) v += reg_add;
    tt[e] = v;
  }
}

#endif  // CUMF_IMPLICIT_PART

#if CUMF_IMPLICIT_PART == 0
// ---- 3. Gram-free CG of short rows (the pattern of als_short.hip, with the weights and G)

// the whole row with at most N entries in flight (N = 8, 16, 32 >= n); TWO: f > 64, the lanes hold two features each;
// Gs: G in LDS at pitch GP (zero columns from f on)
template <bool TWO, int N>
__device__ __forceinline__ void implicit_short_row(const ImplicitArgs& a, const float* Gs, int row, int n, float rv,
                                                   const float* grow, int lane) {
  constexpr int GP = TWO ? 128 : 64;
  const int f = a.f;
  const bool f0 = lane < f, f1 = TWO && lane + 64 < f;
  float* xg = a.update + (size_t)row * f;
  if (n == 0) {  // no stored entry: x = 0 (b = 0)
    if (f0) xg[lane] = 0.f;
    if (f1) xg[64 + lane] = 0.f;
    return;
  }
  float x0 = f0 ? xg[lane] : 0.f, x1 = f1 ? xg[64 + lane] : 0.f;  // warm start (cg.cu:48)
  float T0[N], T1[N];
  const unsigned long long gaddr = reinterpret_cast<unsigned long long>(grow);
  const int glo = (int)(unsigned)gaddr, ghi = (int)(unsigned)(gaddr >> 32);
  static_for<N>([&](auto rc) {
    constexpr int r = decltype(rc)::value;
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane(glo, r), hi = (unsigned)__builtin_amdgcn_readlane(ghi, r);
    typedef __attribute__((address_space(1))) const float gfloat;  // global loads, not flat ones
    gfloat* base = reinterpret_cast<gfloat*>(((unsigned long long)hi << 32) | lo);
    T0[r] = f0 ? base[lane] : 0.f;
    T1[r] = f1 ? base[64 + lane] : 0.f;
  });
  const bool live = lane < n;
  const float wv = live ? a.alpha * fabsf(rv) : 0.f;            // confidence weight of entry `lane`
  const float cv = (live && rv > 0.f) ? 1.f + wv : 0.f;         // its coefficient in b
  const float reg = a.reg_mode == kImpRegPlain ? a.lambda : (float)n * a.lambda;
  // y += T^T w for a rating-layout vector w (lane r: w_r)
  auto tt_product = [&](float w, float& y0, float& y1) {
    static_for<N / 4>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      if (4 * q < n) {  // uniform
        static_for<4>([&](auto ic) {
          constexpr int r = 4 * q + decltype(ic)::value;
          const float wr = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, w), r));
          y0 = fmaf(T0[r], wr, y0);
          if constexpr (TWO) y1 = fmaf(T1[r], wr, y1);
        });
      }
    });
  };
  // y = A v = reg v + G v + T^T (w o (T v))
  auto matvec = [&](float v0, float v1, float& y0, float& y1) {
    float P[N];
    static_for<N>([&](auto rc) {
      constexpr int r = decltype(rc)::value;
      P[r] = TWO ? fmaf(T1[r], v1, T0[r] * v0) : T0[r] * v0;
    });
    const float u = reduce_transposed<N>(P, lane) * wv;
    y0 = reg * v0, y1 = reg * v1;
    const int f_lo = f < 64 ? f : 64;
    for (int j = 0; j < f_lo; ++j) {  // G symmetric: (G v)_k = sum_j G[j][k] v_j, row j of G across the lanes
      const float vj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v0), j));
      y0 = fmaf(Gs[j * GP + lane], vj, y0);
      if constexpr (TWO) y1 = fmaf(Gs[j * GP + 64 + lane], vj, y1);
    }
    if constexpr (TWO) {
      for (int j = 64; j < f; ++j) {
        const float vj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v1), j - 64));
        y0 = fmaf(Gs[j * GP + lane], vj, y0);
        y1 = fmaf(Gs[j * GP + 64 + lane], vj, y1);
      }
    }
    tt_product(u, y0, y1);
  };
  auto dot = [&](float a0, float a1, float c0, float c1) { return wave_sum_uniform(TWO ? fmaf(a1, c1, a0 * c0) : a0 * c0); };
  float b0 = 0.f, b1 = 0.f;
  tt_product(cv, b0, b1);  // b = sum_{r > 0} (1 + w) y
  // ---- CG (cg.cu:36-231)
  float ap0, ap1;
  matvec(x0, x1, ap0, ap1);
  float r0 = b0 - ap0, r1 = b1 - ap1;
  float p0 = r0, p1 = r1;
  float rsold = dot(r0, r1, r0, r1);
  for (int iter = 0; iter < a.cg_iters; ++iter) {
    matvec(p0, p1, ap0, ap1);
    const float pap = dot(p0, p1, ap0, ap1);
    const float alpha = rsold / pap;
    x0 = fmaf(alpha, p0, x0), x1 = fmaf(alpha, p1, x1);
    r0 = fmaf(-alpha, ap0, r0), r1 = fmaf(-alpha, ap1, r1);
    const float rsnew = dot(r0, r1, r0, r1);
    if ((double)rsnew < 1e-4) break;  // CG_ERROR (cg.cu:31,195)
    const float beta = rsnew / rsold;
    rsold = rsnew;
    p0 = fmaf(beta, p0, r0), p1 = fmaf(beta, p1, r1);
  }
  if (f0) xg[lane] = x0;
  if (f1) xg[64 + lane] = x1;
}

// zeros that stand in for the factor row of a lane without an entry
static __device__ __attribute__((aligned(16))) float g_imp_zeros[128];

// items [first, first + count) of the plan's list; each wave walks its rows, the workgroup shares G
template <bool TWO>
__global__ __launch_bounds__(kImpThreads) void implicit_short_cg_kernel(const ImplicitArgs a, long long first,
                                                                        long long count) {
  constexpr int GP = TWO ? 128 : 64;
  extern __shared__ float Gs[];
  const int f = a.f;
  for (int e = threadIdx.x; e < f * GP; e += kImpThreads) {
    const int i = e / GP, c = e - i * GP;
    Gs[e] = c < f ? a.G[i * f + c] : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (long long k = (long long)blockIdx.x * 4 + wave; k < count; k += (long long)gridDim.x * 4) {
    const long long item = first + k;
    const int row = a.item_row[item];
    const long long begin = a.item_begin[item];
    const int n = a.item_len[item];  // the whole row (uniform)
    const bool live = lane < n;
    const int j = live ? a.colidx[begin + lane] : 0;
    const float rv = live ? a.val[begin + lane] : 0.f;
    const float* grow = live ? a.gather + (size_t)j * f : g_imp_zeros;
    if (n <= 8)
      implicit_short_row<TWO, 8>(a, Gs, row, n, rv, grow, lane);
    else if (n <= 16)
      implicit_short_row<TWO, 16>(a, Gs, row, n, rv, grow, lane);
    else
      implicit_short_row<TWO, 32>(a, Gs, row, n, rv, grow, lane);
  }
}

// ---- row moves of the long-row CG route

// scatter = 0: out[k] = in[rows[k]]; scatter = 1: out[rows[k]] = in[k]; rows of f floats
__global__ __launch_bounds__(kImpThreads) void implicit_copy_rows_kernel(const int* __restrict__ rows, long long count, int f,
                                                                         const float* __restrict__ in, float* __restrict__ out,
                                                                         int scatter) {
  const long long total = count * f;
  for (long long e = (long long)blockIdx.x * kImpThreads + threadIdx.x; e < total; e += (long long)gridDim.x * kImpThreads) {
    const long long k = e / f, c = e - k * f;
    if (scatter)
      out[(size_t)rows[k] * f + c] = in[e];
    else
      out[e] = in[(size_t)rows[k] * f + c];
  }
}

__global__ __launch_bounds__(kImpThreads) void implicit_zero_rows_kernel(const int* __restrict__ rows, long long count, int f,
                                                                         float* __restrict__ x) {
  const long long total = count * f;
  for (long long e = (long long)blockIdx.x * kImpThreads + threadIdx.x; e < total; e += (long long)gridDim.x * kImpThreads)
    x[(size_t)rows[e / f] * f + e % f] = 0.f;
}

// ---- 4. the objective

// part[block] = sum over its rows' stored entries of (1 + w)(p - s)^2 - s^2 (+ lambda (|x_u|^2 + |y_i|^2) when the
// regulariser is weighted): the pass of als_loss.h, shared with the weighted objective (als_weighted.hip)
__global__ __launch_bounds__(kImpThreads) void implicit_loss_sparse_kernel(const int* __restrict__ rowptr,
                                                                           const int* __restrict__ colidx,
                                                                           const float* __restrict__ val,
                                                                           const float* __restrict__ XT,
                                                                           const float* __restrict__ thetaT, long long m,
                                                                           int f, float lambda, float alpha, int reg_mode,
                                                                           double* __restrict__ part) {
  const double alp = alpha;
  loss_sparse_pass(rowptr, colidx, XT, thetaT, m, f, lambda, reg_mode != kImpRegPlain, part, [&](long long k, double s) {
    const double r = val[k];
    const double w = alp * fabs(r), p = r > 0.0 ? 1.0 : 0.0;
    return (1.0 + w) * (p - s) * (p - s) - s * s;
  });
}

// out = sum of the parts + <Gx, Gy>_F (+ lambda (tr Gx + tr Gy) when the regulariser is plain)
__global__ __launch_bounds__(kImpThreads) void implicit_loss_final_kernel(const double* __restrict__ part, int nparts,
                                                                          const double* __restrict__ Gx,
                                                                          const double* __restrict__ Gy, int f, float lambda,
                                                                          int reg_mode, double* __restrict__ out) {
  __shared__ double red[kImpThreads];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kImpThreads) acc += part[i];
  for (int e = threadIdx.x; e < f * f; e += kImpThreads) acc += Gx[e] * Gy[e];
  if (reg_mode == kImpRegPlain)
    for (int i = threadIdx.x; i < f; i += kImpThreads) acc += (double)lambda * (Gx[i * f + i] + Gy[i * f + i]);
  const double t = loss_block_sum(acc, red);
  if (threadIdx.x == 0) out[0] = t;
}

static unsigned grid_for(long long work, long long per_block, long long cap) {
  const long long g = (work + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

size_t implicit_gram_part_floats(long rows, int f) {
  const size_t FP = 16 * (size_t)((f + 15) / 16);
  const long slab = implicit_gram_slab(f);
  return (size_t)((rows + slab - 1) / slab) * FP * FP;
}

hipError_t launch_implicit_gram_reduce(const float* part, long rows, int f, float* G, double* G64, hipStream_t stream) {
  const long slab = implicit_gram_slab(f);
  const int FT = (f + 15) / 16, nslab = (int)((rows + slab - 1) / slab);
  return launch_kernel(implicit_gram_reduce_kernel, dim3(grid_for((long long)f * f, kImpThreads, 1 << 20)), dim3(kImpThreads), 0,
                       stream, part, nslab, f, 16 * FT, G, G64);
}

hipError_t launch_implicit_gram(const float* Y, long rows, int f, float* part, float* G, double* G64, hipStream_t stream) {
  const long slab = implicit_gram_slab(f);
  const int FT = (f + 15) / 16, nslab = (int)((rows + slab - 1) / slab);
  if (nslab > 0 && FT > 8) {  // 128 < f <= 512: the tiles spread over a second grid dimension (als_implicit_free.hip)
    const hipError_t e = launch_implicit_gram_wide(Y, nullptr, rows, f, part, stream);
    if (e != hipSuccess) return e;
  } else if (nslab > 0) {
    const hipError_t e = with_nb<1, 8>(FT, [&](auto ft) {
      return launch_kernel(implicit_gram_partial_kernel<decltype(ft)::value>, dim3((unsigned)nslab), dim3(kImpThreads), 0,
                           stream, Y, (long long)rows, f, part);
    });
    if (e != hipSuccess) return e;
  }
  return launch_implicit_gram_reduce(part, rows, f, G, G64, stream);
}

hipError_t launch_implicit_hermitian(const ImplicitArgs& a, long n_items, long n_mrows, hipStream_t stream) {
  if (n_items > 0) {
    const hipError_t e = with_nb<1, 8>((a.f + 15) / 16, [&](auto ft) {
      return launch_item_kernel(implicit_hermitian_kernel<decltype(ft)::value>, dim3((unsigned)n_items), dim3(kImpThreads), 0,
                                stream, a);
    });
    if (e != hipSuccess) return e;
  }
  if (n_mrows > 0)
    return launch_kernel(implicit_slot_reduce_kernel, dim3((unsigned)n_mrows), dim3(kImpThreads), 0, stream, a);
  return hipSuccess;
}

hipError_t launch_implicit_short_cg(const ImplicitArgs& a, long first, long count, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  const bool two = a.f > 64;
  const size_t lds = (size_t)a.f * (two ? 128 : 64) * sizeof(float);
  return launch_item_kernel(two ? implicit_short_cg_kernel<true> : implicit_short_cg_kernel<false>,
                            dim3(grid_for(count, 4, 8192)), dim3(kImpThreads), lds, stream, a, (long long)first,
                            (long long)count);
}

hipError_t launch_implicit_copy_rows(const int* rows, long count, int f, const float* in, float* out, bool scatter,
                                     hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  return launch_kernel(implicit_copy_rows_kernel, dim3(grid_for((long long)count * f, kImpThreads, 16384)), dim3(kImpThreads), 0,
                       stream, rows, (long long)count, f, in, out, (int)scatter);
}

hipError_t launch_implicit_zero_rows(const int* rows, long count, int f, float* x, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  return launch_kernel(implicit_zero_rows_kernel, dim3(grid_for((long long)count * f, kImpThreads, 16384)), dim3(kImpThreads), 0,
                       stream, rows, (long long)count, f, x);
}

hipError_t launch_implicit_loss(const int* rowptr, const int* colidx, const float* val, const float* XT, const float* thetaT,
                                long m, int f, float lambda, float alpha, int reg_mode, const double* Gx, const double* Gy,
                                double* part, double* out, hipStream_t stream) {
  hipError_t e = launch_kernel(implicit_loss_sparse_kernel, dim3(kImpLossBlocks), dim3(kImpThreads), 0, stream, rowptr, colidx,
                               val, XT, thetaT, (long long)m, f, lambda, alpha, reg_mode, part);
  if (e != hipSuccess) return e;
  return launch_kernel(implicit_loss_final_kernel, dim3(1), dim3(kImpThreads), 0, stream, (const double*)part,
                       (int)kImpLossBlocks, Gx, Gy, f, lambda, reg_mode, out);
}

#elif CUMF_IMPLICIT_PART == 1

hipError_t launch_implicit_partial(const ImplicitArgs& a, long n_items, long n_mrows, hipStream_t stream) {
  if (n_items > 0) {
    const hipError_t e = with_nb<1, 8>((a.f + 15) / 16, [&](auto ft) {
      return launch_item_kernel(implicit_hermitian_kernel<kImpPacked + decltype(ft)::value>, dim3((unsigned)n_items),
                                dim3(kImpThreads), 0, stream, a);
    });
    if (e != hipSuccess) return e;
  }
  if (n_mrows > 0)
    return launch_kernel(implicit_slot_reduce_packed_kernel, dim3((unsigned)n_mrows), dim3(kImpThreads), 0, stream, a);
  return hipSuccess;
}

hipError_t launch_implicit_finish(const float* packed, const float* G, float reg_add, float* tt, long batch, int f,
                                  hipStream_t stream) {
  if (batch <= 0) return hipSuccess;
  const long long blocks = ((long long)batch * f * f + kImpThreads - 1) / kImpThreads;
  return launch_kernel(implicit_finish_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(kImpThreads), 0, stream,
                       packed, G, reg_add, tt, (long long)batch, f);
}

#else  // CUMF_IMPLICIT_PART == 2

// G = Y^T diag(row_w) Y: implicit_gram_partial_kernel with the stage's weights beside it in LDS and the weighted form of the
// stage product the item kernel uses (implicit_stage_tiles<FT, true>: the A operand of table row k is row_w[k] y_k; at
// row_w = 1 the operand itself, so the partials are implicit_gram_partial_kernel's bits)
template <int FT>
__global__ __launch_bounds__(kImpThreads) void weighted_gram_partial_kernel(const float* __restrict__ Y,
                                                                            const float* __restrict__ row_w, long long rows,
                                                                            int f, float* __restrict__ part) {
  constexpr int FP = 16 * FT, TPW = ImplicitTiles<FT>::TPW, NT = ImplicitTiles<FT>::NT;
  __shared__ float ys[kImpStage * implicit_stage_pitch(FP)];
  __shared__ float sw[kImpStage];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const ImplicitTiles<FT> T(wave);
  f32x4 acc[TPW];
#pragma unroll
  for (int q = 0; q < TPW; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  const long long r0 = (long long)blockIdx.x * kImpGramSlab;
  const int n = (int)(rows - r0 < kImpGramSlab ? rows - r0 : kImpGramSlab);
  for (int s = 0; s < n; s += kImpStage) {
    const int cnt = n - s < kImpStage ? n - s : kImpStage;
    __syncthreads();
    implicit_load_stage<FP>(ys, cnt, f, [&](int r) { return Y + (size_t)(r0 + s + r) * f; });
    if ((int)threadIdx.x < kImpStage) sw[threadIdx.x] = (int)threadIdx.x < cnt ? row_w[r0 + s + threadIdx.x] : 0.f;
    __syncthreads();
    implicit_stage_tiles<FT, true>(ys, sw, T, acc, wave, lane);
  }
  float* out = part + (size_t)blockIdx.x * FP * FP;
#pragma unroll
  for (int q = 0; q < TPW; ++q) {
    if (wave + 4 * q < NT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(16 * T.I[q] + 4 * (lane >> 4) + r) * FP + 16 * T.J[q] + (lane & 15)] = acc[q][r];
    }
  }
}

// launch_implicit_gram with a weight per table row: the same slabs, stages, tile order and reduce
hipError_t launch_weighted_gram(const float* Y, const float* row_w, long rows, int f, float* part, float* G, double* G64,
                                hipStream_t stream) {
  const long slab = implicit_gram_slab(f);
  const int FT = (f + 15) / 16, nslab = (int)((rows + slab - 1) / slab);
  if (nslab > 0 && FT > 8) {
    const hipError_t e = launch_implicit_gram_wide(Y, row_w, rows, f, part, stream);
    if (e != hipSuccess) return e;
  } else if (nslab > 0) {
    const hipError_t e = with_nb<1, 8>(FT, [&](auto ft) {
      return launch_kernel(weighted_gram_partial_kernel<decltype(ft)::value>, dim3((unsigned)nslab), dim3(kImpThreads), 0,
                           stream, Y, row_w, (long long)rows, f, part);
    });
    if (e != hipSuccess) return e;
  }
  return launch_implicit_gram_reduce(part, rows, f, G, G64, stream);
}

#endif  // CUMF_IMPLICIT_PART

}  // namespace cumf
