// als_wg_solve.h -- the solvers of the workgroup kernels (als_kernels.hip) on a system in LDS: CG and the oracle-order LU
// on a full G, the loaders that hand a system to the register LU (als_lu_reg.h), and where the LU runs on the accumulators
// instead (als_lu_wg.h).
#ifndef CUMF_ALS_WG_SOLVE_H_
#define CUMF_ALS_WG_SOLVE_H_

#include <hip/hip_runtime.h>

#include "als_device.h"
#include "als_internal.h"
#include "als_lu_reg.h"
#include "als_lu_wg.h"

namespace cumf {

// The accumulator LU pays off from f = 96 on (measured: f = 64 18.8 vs 18.0 ms, f = 10 0.67 vs 0.56 ms with
// the thread-grid LU; f = 100 35.7 vs 36.8, f = 128 62.2 vs 63.8, f = 200 200 vs 224).
constexpr bool lu_on_accumulators(int nb) { return nb >= 7; }

// ----------------------------------------------------------------------------------
// In-LDS solvers.  G is f x ldg (ldg = solve_ldg(f): f + 1 rounded up to 4, so rows
// are 16-byte aligned), column f holds b.  256 threads.
// ----------------------------------------------------------------------------------

// Conjugate gradient exactly as cg.cu:36-231: warm start, r = b - A x, <= cg_iters
// iterations, stop when ||r||^2 < 1e-4 (CG_ERROR, cg.cu:31,195; the float is compared
// against the double literal).
//
// Layout: every wave keeps ALL four vectors (x, r, p, ap) in registers, element i in lane
// i & 63, slot i >> 6, and performs the vector updates and the dot products redundantly;
// identical instruction sequences on identical data give identical bits in the four
// waves, so alpha / beta / the exit test are workgroup-uniform without communication.
// Only the mat-vec is shared: wave w multiplies rows [w*JW, (w+1)*JW) of the symmetric G
// (16-byte LDS reads, both half-waves on different rows), the four partial vectors go
// through LDS and ONE barrier per iteration.  Dot products are fixed-order DPP
// reductions in place of the reference's order-dependent smem atomics
// (device_utilities.h:36-48).  Requires f <= 128.
template <int NB>
__device__ __forceinline__ void cg_solve_lds(const float* __restrict__ G, int ldg, int f,
                                             float* __restrict__ vec, float* __restrict__ x_global,
                                             int cg_iters, int tid) {
  constexpr int MAXIT = 2 * NB;  // rows per half-wave: ceil(ceil(16*NB / 4) / 2)
  const int wave = tid >> 6, lane = tid & 63;
  const int c = lane & 31, h = lane >> 5;
  float* pw = vec + wave * kVecLd;      // this wave's private copy of the mat-vec operand
  float* part = vec + 4 * kVecLd;       // [2][4][kVecLd] partial mat-vecs, double-buffered
  const int jw = (f + 3) >> 2;          // rows of G per wave
  const int jbeg = wave * jw;
  const int jend = (jbeg + jw) < f ? (jbeg + jw) : f;
  const bool colok = 4 * c < ldg;
  const int i0 = lane, i1 = lane + 64;
  const bool ok0 = i0 < f, ok1 = i1 < f;

  int buf = 0;
  // y = G * v for the vector held as (v0, v1); result replicated in every wave
  auto matvec = [&](float v0, float v1, float& y0, float& y1) {
    pw[i0] = v0;
    pw[i1] = v1;
    __builtin_amdgcn_wave_barrier();
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int j = jbeg + h + 2 * it;
      const bool on = (j < jend) && colok;
      const int jc = on ? j : 0;
      const f32x4 g = *reinterpret_cast<const f32x4*>(G + jc * ldg + (on ? 4 * c : 0));
      const float pj = on ? pw[jc] : 0.f;
      acc[0] = fmaf(g[0], pj, acc[0]);
      acc[1] = fmaf(g[1], pj, acc[1]);
      acc[2] = fmaf(g[2], pj, acc[2]);
      acc[3] = fmaf(g[3], pj, acc[3]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] += __shfl_xor(acc[e], 32);
    float* pb = part + (buf * 4 + wave) * kVecLd;
    if (h == 0) *reinterpret_cast<f32x4*>(pb + 4 * c) = acc;
    __syncthreads();
    const float* pr = part + buf * 4 * kVecLd;
    y0 = ((pr[i0] + pr[kVecLd + i0]) + pr[2 * kVecLd + i0]) + pr[3 * kVecLd + i0];
    y1 = ((pr[i1] + pr[kVecLd + i1]) + pr[2 * kVecLd + i1]) + pr[3 * kVecLd + i1];
    buf ^= 1;
  };

  float x0 = ok0 ? x_global[i0] : 0.f, x1 = ok1 ? x_global[i1] : 0.f;
  float ax0, ax1;
  matvec(x0, x1, ax0, ax1);
  float r0 = ok0 ? G[i0 * ldg + f] - ax0 : 0.f;
  float r1 = ok1 ? G[i1 * ldg + f] - ax1 : 0.f;
  float p0 = r0, p1 = r1;
  float rsold = wave_sum_uniform(fmaf(r1, r1, r0 * r0));
  for (int iter = 0; iter < cg_iters; ++iter) {
    float ap0, ap1;
    matvec(p0, p1, ap0, ap1);
    ap0 = ok0 ? ap0 : 0.f;
    ap1 = ok1 ? ap1 : 0.f;
    const float pap = wave_sum_uniform(fmaf(p1, ap1, p0 * ap0));
    const float alpha = rsold / pap;
    x0 = fmaf(alpha, p0, x0);
    x1 = fmaf(alpha, p1, x1);
    r0 = fmaf(-alpha, ap0, r0);
    r1 = fmaf(-alpha, ap1, r1);
    const float rsnew = wave_sum_uniform(fmaf(r1, r1, r0 * r0));
    if ((double)rsnew < 1e-4) break;
    const float beta = rsnew / rsold;
    rsold = rsnew;
    p0 = fmaf(beta, p0, r0);
    p1 = fmaf(beta, p1, r1);
  }
  if (wave == 0) {
    if (ok0) x_global[i0] = x0;
    if (ok1) x_global[i1] = x1;
  }
}

// Back substitution U x = y by one wave (lanes own rows i = lane + 64 q), column-oriented
// like BLAS strsv: x_k final, then every y_i (i < k) loses U_ik x_k.  rdiag (may be null)
// holds the reciprocals of the pivots; without it x_k = y_k / U_kk (IEEE division).
template <bool RECIP, int NQ>
__device__ __forceinline__ void back_substitute_lds(const float* __restrict__ G, int ldg, int f,
                                                    const float* __restrict__ rdiag,
                                                    float* __restrict__ x_global, int lane) {
  float y[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) y[q] = (lane + 64 * q < f) ? G[(lane + 64 * q) * ldg + f] : 0.f;
  // column k of U for this lane's rows, fetched one step ahead of its use
  float col[NQ], coln[NQ];
  float dk = 0.f, dkn = 0.f;
  const float* colp[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = lane + 64 * q;
    colp[q] = G + (i < f ? i : f - 1) * ldg;
  }
  auto fetch = [&](int k, float (&cv)[NQ], float& d) {
    const int kc = k < 0 ? 0 : k;
#pragma unroll
    for (int q = 0; q < NQ; ++q) cv[q] = colp[q][kc];
    d = RECIP ? rdiag[kc] : G[kc * ldg + kc];
  };
  fetch(f - 1, col, dk);
  for (int k = f - 1; k >= 0; --k) {
    fetch(k - 1, coln, dkn);
    const int kq = k >> 6, kl = k & 63;
    float yk = 0.f;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (q == kq) yk = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, y[q]), kl));
    const float xk = RECIP ? yk * dk : yk / dk;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int i = lane + 64 * q;
      const float upd = fmaf(-col[q], xk, y[q]);
      y[q] = (i == k) ? xk : ((i < k) ? upd : y[q]);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) col[q] = coln[q];
    dk = dkn;
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    if (lane + 64 * q < f) x_global[lane + 64 * q] = y[q];
}

// Unpivoted Gaussian elimination on the augmented system [A | b] followed by back
// substitution: the mathematical content of cublasSgetrfBatched(PivotArray = NULL) +
// cublasSgetrsBatched (als.cu:77,98), all in LDS.  Same operation order as oracle_lu
// (right-looking, IEEE division by the pivot, fmaf updates, descending back
// substitution), so the result is bit-identical to the oracle on identical A, b.  LDS
// bandwidth bound; kept for f > 128 (any ldg) and as the exact-order reference variant.
__device__ __forceinline__ void lu_solve_lds(float* __restrict__ G, int ldg, int f,
                                             float* __restrict__ x_global, int tid) {
  const int ti = tid >> 4, tj = tid & 15;
  for (int k = 0; k < f; ++k) {
    const float piv = G[k * ldg + k];
    for (int i = k + 1 + tid; i < f; i += kThreads) G[i * ldg + k] = G[i * ldg + k] / piv;
    __syncthreads();
    for (int i = k + 1 + ti; i < f; i += 16) {
      const float l = G[i * ldg + k];
      for (int j = k + 1 + tj; j <= f; j += 16) G[i * ldg + j] = fmaf(-l, G[k * ldg + j], G[i * ldg + j]);
    }
    __syncthreads();
  }
  if (tid < 64) back_substitute_lds<false, 4>(G, ldg, f, nullptr, x_global, tid);
}

// Register-resident symmetric elimination (lu_solve_reg): als_lu_reg.h.

// LDS floats of the fused LU of NB feature blocks: lu_solve_mfma (NB >= 7) or the thread-grid
// lu_solve_reg on the packed row store.
template <int NB>
__host__ __device__ constexpr size_t lu_fused_lds_floats(int f) {
  return lu_on_accumulators(NB) ? lu_wg_lds_floats<NB>(f) : lu_lds_floats(NB, f);
}

// Loaders of lu_solve_reg.  TileLoad: the accumulator tiles parked in LDS by tiles_to_tiled.
template <int NB>
struct TileLoad {
  const float* T;
  int f;
  template <typename BI, typename BJ>
  __device__ __forceinline__ float operator()(BI, BJ, int ti, int tj) const {
    constexpr int bi = BI::value, bj = BJ::value;
    const int i = 16 * bi + ti, j = 16 * bj + tj;
    const float v = T[256 * tile_of<NB>(bi, bj) + tiled_row(ti) * 16 + tj];
    return (i < f && j <= f) ? v : 0.f;
  }
};
// GlobalLoad: a row-major f x f matrix and its right-hand side in global memory.
template <int NB>
struct GlobalLoad {
  const float* A;
  const float* b;
  int f;
  template <typename BI, typename BJ>
  __device__ __forceinline__ float operator()(BI, BJ, int ti, int tj) const {
    constexpr int bi = BI::value, bj = BJ::value;
    const int i = 16 * bi + ti, j = 16 * bj + tj;
    const int ic = i < f ? i : f - 1;
    const float v = (j < f) ? A[(size_t)ic * f + j] : b[ic];
    return (i < f && j <= f) ? v : 0.f;
  }
};

}  // namespace cumf

#endif  // CUMF_ALS_WG_SOLVE_H_
