// als_lu_reg.h -- the register-resident symmetric elimination of the batched LU (lu_solve_reg), shared by
// als_kernels.hip (cumf_lu_solve_batched and the fused LU of NB < 7) and als_nnls.hip (the passive-set solves of the
// NNLS kernel, through a masking loader).
#ifndef CUMF_ALS_LU_REG_H_
#define CUMF_ALS_LU_REG_H_

#include <hip/hip_runtime.h>

#include "als_internal.h"
#include "als_device.h"

namespace cumf {

// Register-resident symmetric elimination (the fast LU path, f <= 200).
// The upper triangle of [A | b] is spread over the 16 x 16 thread grid, element (i, j) in
// thread (i & 15, j & 15), register block (i >> 4, j >> 4); `load(bi, bj)` fetches this
// thread's element of block (bi, bj) (from the accumulator tiles parked in LDS, or from
// global memory).  Per pivot k:
//   1. the thread row owning row k publishes it (as it stands, i.e. updated by all earlier
//      pivots) to the packed row store U (lu_row_off); the thread holding u_kk computes
//      1 / u_kk meanwhile and publishes that too, so the reciprocal is off the readers'
//      critical path; ONE barrier;
//   2. every thread reads row k at its own row / column positions and applies
//      a_ij -= (u_ki / u_kk) * u_kj  to its registers (i > k).
// This is Gaussian elimination without pivoting restricted to the upper triangle (U = D L^T of
// A = L U).  Tried and measured slower or equal: panels of 2 or 4
// pivots per barrier with a redundant in-register panel elimination (half / quarter the
// barriers, same LDS reads: equal at M = 2, spills at M = 4), a rolled pivot loop (+5 %).
// U may alias the memory `load` reads from: all loads complete before the first publish.
template <int NB, typename Load>
__device__ __forceinline__ void lu_solve_reg(Load load, float* __restrict__ U, int f, float* __restrict__ rdiag,
                                             float* __restrict__ x_global, int tid) {
  const int ti = tid >> 4, tj = tid & 15;
  float* zpad = rdiag + ((f + 3) & ~3) + 32;  // 16 zeros for back_substitute_zeroed (same place as in lu_solve_mfma)
  if (tid < 16) zpad[tid] = 0.f;
  float a[NB][NB];
  static_for<NB>([&](auto bic) {
    constexpr int bi = decltype(bic)::value;
    static_for<NB>([&](auto bjc) {
      constexpr int bj = decltype(bjc)::value;
      if constexpr (bj >= bi) a[bi][bj] = load(bic, bjc, ti, tj);
    });
  });
  __syncthreads();
  // Rows >= f and columns > f of the register image are padding: never published, never read
  // back, so updates run on them unmasked (whatever lands there is dead).  Reads of padding
  // positions stay inside the row store and only feed dead registers.
  const bool last_col_ok = 16 * (NB - 1) + tj <= f;
  static_for<NB>([&](auto kbc) {
    constexpr int kb = decltype(kbc)::value;
    constexpr int pitch = lu_row_pitch<NB>(kb);
    float* blk = U + lu_block_off<NB>(kb) - 16 * kb;  // element (16 kb, 0) of this block row
    for (int kk = 0; kk < 16; ++kk) {
      const int k = 16 * kb + kk;
      if (k >= f) break;
      float* urow = blk + kk * pitch;
      if (ti == kk) {
        float* w = urow + tj;
        static_for<NB>([&](auto bjc) {
          constexpr int bj = decltype(bjc)::value;
          // entries at or left of the diagonal inside the row's own block are dead for the
          // elimination: publish zeros there, the back substitution then needs no triangle mask
          const float v = (bj > kb || tj > kk) ? a[kb][bj] : 0.f;
          if constexpr (bj >= kb && bj < NB - 1) w[16 * bj] = v;
          if constexpr (bj >= kb && bj == NB - 1) {
            if (last_col_ok) w[16 * bj] = v;
          }
        });
        if (tj == kk) {
          const float piv = a[kb][kb];
          const float t = __builtin_amdgcn_rcpf(piv);
          rdiag[k] = fmaf(fmaf(-piv, t, 1.0f), t, t);  // one Newton step: 1/pivot to ~1 ulp
        }
      }
      __syncthreads();
      float ui[NB], uj[NB];
      const float nrp = -rdiag[k];
      static_for<NB>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        if constexpr (b >= kb) {
          uj[b] = urow[16 * b + tj];
          ui[b] = urow[16 * b + ti];
        }
      });
      static_for<NB>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        if constexpr (b > kb) ui[b] = ui[b] * nrp;
        if constexpr (b == kb) ui[b] = (ti > kk) ? ui[b] * nrp : 0.f;
      });
      static_for<NB>([&](auto bic) {
        constexpr int bi = decltype(bic)::value;
        static_for<NB>([&](auto bjc) {
          constexpr int bj = decltype(bjc)::value;
          if constexpr (bi >= kb && bj >= bi) a[bi][bj] = fmaf(ui[bi], uj[bj], a[bi][bj]);
        });
      });
    }
  });
  __syncthreads();
  if (tid < 64) back_substitute_zeroed<NB, (16 * NB + 63) / 64>(U, f, rdiag, zpad, x_global, tid);
}

}  // namespace cumf

#endif  // CUMF_ALS_LU_REG_H_
