// als_block_core.h -- the device core of the block Gauss-Seidel solvers (als_block.h): what the kernels of the segmented
// route (als_block.hip: one wave per segment, partials and yhat in global memory) and the fused kernels
// (als_block_fused.hip, als_block_gram.hip: one wave per row, everything on chip) share, so that all sum the same terms in the
// same order.
//   block_entry_weight  the weight and coefficient of a stored entry in each weight mode, as free_sparse_pass forms them;
//   block_open_pass     yhat_e = t_e . x of a run of entries by the transposing wave reduction (lane l holds features l + 64 q);
//   block_accumulate64  at most 64 entries of a block step, four at a time: lane i + 16 kappa loads the two 64-byte half-slices
//                       of entry kappa as v_mfma_f32_16x16x4_f32 operands, folds the previous block's step into yhat (16-lane
//                       DPP row sum) and accumulates g on the VALU and H00 | H01 | H11 on the matrix pipe, K in entry order;
//   block_tile_put      one element of the tiles into the 32 x 33 LDS tile, mirrored, reg on the live diagonal;
//   block_partials_to_tile  the segment partials of a row summed in segment order and scattered with block_tile_put;
//   block_solve32       the 32 x 32 system eliminated without pivoting in registers: lane i holds row i, the pivot row goes
//                       round by v_readlane; the step d comes back in lanes 0..31, repeated in lanes 32..63;
//   block_nnls32        the same 32 x 32 system under z >= 0 by block principal pivoting: the passive set is a 32-bit mask in
//                       SGPRs, every step is block_solve32 on the masked system re-read from the LDS tile.
#ifndef CUMF_ALS_BLOCK_CORE_H_
#define CUMF_ALS_BLOCK_CORE_H_

#include <hip/hip_runtime.h>

#include "als_block.h"
#include "als_free_core.h"

namespace cumf {

// the sum over the 16 lanes of each DPP row, in every lane of the row
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_term<0xB1, 0xf>(v);   // quad_perm [1,0,3,2]
  v += dpp_term<0x4E, 0xf>(v);   // quad_perm [2,3,0,1]
  v += dpp_term<0x141, 0xf>(v);  // row_half_mirror
  v += dpp_term<0x140, 0xf>(v);  // row_mirror
  return v;
}
__device__ __forceinline__ float read_lane(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// ---- yhat of the `len` entries from `begin` on against v (lane l: features l + 64 q); put(offset from begin, yhat) is
// called by the lane that ends up with the entry's sum
template <int Q, class Put>
__device__ __forceinline__ void block_open_pass(const BlockArgs& a, long long begin, int len, const float (&v)[Q], int lane,
                                                Put&& put) {
  constexpr int N = Q <= 4 ? 16 : 8;  // entries per transposing reduction
  const int f = a.f;
  for (int s = 0; s < len; s += 64) {
    const int cnt64 = len - s < 64 ? len - s : 64;
    const int jl = lane < cnt64 ? a.colidx[begin + s + lane] : 0;
    for (int b = 0; b < cnt64; b += N) {
      const int cnt = cnt64 - b < N ? cnt64 - b : N;  // uniform
      float P[N];
      static_for<N>([&](auto rc) {
        constexpr int r = decltype(rc)::value;
        float d = 0.f;
        if (r < cnt) {
          const float* y = a.gather + (size_t)__builtin_amdgcn_readlane(jl, b + r) * f;
          d = (lane < f ? y[lane] : 0.f) * v[0];
#pragma unroll
          for (int q = 1; q < Q; ++q) d = fmaf(lane + 64 * q < f ? y[lane + 64 * q] : 0.f, v[q], d);
        }
        P[r] = d;
      });
      const float u = reduce_transposed<N>(P, lane);  // lane L: entry b + (L mod N)
      if (lane < cnt) put(s + b + lane, u);
    }
  }
}

// ---- the accumulators of a block step: the tiles in MFMA layout (lane i + 16 kappa, element r: row 4 kappa + r, column i) and
// the lane groups' parts of g[i] and g[16 + i]
struct BlockAcc {
  f32x4 H00, H01, H11;
  float g0, g1;
};
__device__ __forceinline__ BlockAcc block_acc_zero() {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  return BlockAcc{z, z, z, 0.f, 0.f};
}
// the block [c0, c0 + 32) of step k and the block before it (k - 1, or the last block when k = 0), with the lanes' masks: a
// ragged last block reads zeros beyond f
struct BlockCols {
  int c0, p0;
  bool v0, v1, pv0, pv1;
};
__device__ __forceinline__ BlockCols block_cols(int f, int k, int i) {
  constexpr int B = kBlockWidth;
  const int c0 = B * k, p0 = B * (k > 0 ? k - 1 : (f + B - 1) / B - 1);
  return BlockCols{c0, p0, c0 + i < f, c0 + 16 + i < f, p0 + i < f, p0 + 16 + i < f};
}

// The weight wl and coefficient cl of stored entry e (column jl, rating rl) in a live lane, formed as free_sparse_pass forms
// them.  kFreeWeightAlpha: the confidence weight a.alpha |r| and (1 + w) p; kFreeWeightArray: q_e = wgt[e] - a.w0 and w_e r_e;
// kFreeWeightRank1: q_e = fma(-aw, gather_w0[jl], wgt[e]) (aw = own_w0 of the row, wave-uniform; one 4-byte gather by the
// column index the lane holds) and w_e r_e.  q_e may be negative.  A lane that is not live gets w = 0 and c = 0.
template <FreeWeight kWeight>
__device__ __forceinline__ void block_entry_weight(const BlockArgs& a, long long e, bool live, int jl, float rl, float aw,
                                                   float& wl, float& cl) {
  wl = 0.f, cl = rl;
  if constexpr (kWeight == kFreeWeightAlpha) {
    wl = live ? a.alpha * fabsf(rl) : 0.f;
    cl = (live && rl > 0.f) ? 1.f + wl : 0.f;
  } else if constexpr (kWeight == kFreeWeightArray) {
    const float gl = live ? a.wgt[e] : 0.f;
    wl = live ? gl - a.w0 : 0.f;
    cl = gl * rl;
  } else if constexpr (kWeight == kFreeWeightRank1) {
    const float gl = live ? a.wgt[e] : 0.f;
    const float cj = live ? a.gather_w0[jl] : 0.f;
    wl = live ? fmaf(-aw, cj, gl) : 0.f;
    cl = gl * rl;
  }
}

// At most 64 entries (cnt64), entry l in lane l: column jl, weight wl (kFreeWeightNone: 1, not read), coefficient cl, cached
// prediction yl.  have_prev: yhat += t[pi_prev] . d of the step before (d0 = d[i], d1 = d[16 + i]) comes first; the return
// value is then the new yhat of entry 4 i + kappa in lane i + 16 kappa.  An entry beyond cnt64 has c = 0 and zero slices.
template <FreeWeight kWeight>
__device__ __forceinline__ float block_accumulate64(const float* gather, int f, const BlockCols& bc, int cnt64, int jl, float wl,
                                                    float cl, float yl, int have_prev, float d0, float d1, int i, int kap,
                                                    BlockAcc& acc) {
  constexpr int U = 4;  // four-entry groups in flight
  float ynew = 0.f;
  const int ngroups = (cnt64 + 3) >> 2;
  for (int g = 0; g < ngroups; g += U) {
    float t0[U], t1[U], q0[U], q1[U];
    static_for<U>([&](auto uc) {
      constexpr int u = decltype(uc)::value;
      const int src = 4 * (g + u) + kap;
      const bool ok = src < cnt64;
      const float* y = gather + (size_t)__shfl(jl, src & 63) * f;
      t0[u] = (ok && bc.v0) ? y[bc.c0 + i] : 0.f;
      t1[u] = (ok && bc.v1) ? y[bc.c0 + 16 + i] : 0.f;
      q0[u] = q1[u] = 0.f;
      if (have_prev) {
        q0[u] = (ok && bc.pv0) ? y[bc.p0 + i] : 0.f;
        q1[u] = (ok && bc.pv1) ? y[bc.p0 + 16 + i] : 0.f;
      }
    });
    static_for<U>([&](auto uc) {
      constexpr int u = decltype(uc)::value;
      if (g + u < ngroups) {  // uniform
        const int src = (4 * (g + u) + kap) & 63;
        [[maybe_unused]] float w = 1.f;
        if constexpr (kWeight != kFreeWeightNone) w = __shfl(wl, src);
        const float c = __shfl(cl, src);
        float y = __shfl(yl, src);
        if (have_prev) {
          y += row16_sum(fmaf(q1[u], d1, q0[u] * d0));
          ynew = g + u == i ? y : ynew;
        }
        if constexpr (kWeight == kFreeWeightNone) {  // w = 1: the A and B operands are the same registers
          const float ce = c - y;
          acc.g0 = fmaf(t0[u], ce, acc.g0);
          acc.g1 = fmaf(t1[u], ce, acc.g1);
          acc.H00 = __builtin_amdgcn_mfma_f32_16x16x4f32(t0[u], t0[u], acc.H00, 0, 0, 0);
          acc.H01 = __builtin_amdgcn_mfma_f32_16x16x4f32(t0[u], t1[u], acc.H01, 0, 0, 0);
          acc.H11 = __builtin_amdgcn_mfma_f32_16x16x4f32(t1[u], t1[u], acc.H11, 0, 0, 0);
        } else {
          const float ce = fmaf(-w, y, c);
          acc.g0 = fmaf(t0[u], ce, acc.g0);
          acc.g1 = fmaf(t1[u], ce, acc.g1);
          const float w0 = w * t0[u], w1 = w * t1[u];
          acc.H00 = __builtin_amdgcn_mfma_f32_16x16x4f32(w0, t0[u], acc.H00, 0, 0, 0);
          acc.H01 = __builtin_amdgcn_mfma_f32_16x16x4f32(w0, t1[u], acc.H01, 0, 0, 0);
          acc.H11 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1, t1[u], acc.H11, 0, 0, 0);
        }
      }
    });
  }
  return ynew;
}
// the four lane groups of g, in group order: every lane group ends with the sum
__device__ __forceinline__ float block_g_sum(float g, int i) {
  return ((__shfl(g, i) + __shfl(g, 16 + i)) + __shfl(g, 32 + i)) + __shfl(g, 48 + i);
}

// ---- the wave's 32 x 33 LDS tile of H.  Element (ri, ci) of tile t (0: H00, 1: H01, 2: H11): the upper triangles of H00 and
// H11 and all of H01 are written, mirrored, with reg on the live diagonal
constexpr int kBlockTilePitch = kBlockWidth + 1;
__device__ __forceinline__ void block_tile_put(float* Hs, int t, int ri, int ci, float h, float reg, int bw) {
  constexpr int HP = kBlockTilePitch;
  const int R = t == 2 ? 16 + ri : ri, C = t == 0 ? ci : 16 + ci;
  if (t == 1 || ci >= ri) {
    Hs[R * HP + C] = (R == C && R < bw) ? h + reg : h;
    if (R != C) Hs[C * HP + R] = h;
  }
}
// the `ns` consecutive partials from `part` on (kBlockPart floats each) summed in segment order into the tile; returns g[lane]
// in lanes 0..31
__device__ __forceinline__ float block_partials_to_tile(const float* part, int ns, float* Hs, int lane, float reg, int bw) {
  float hp[12], gp = 0.f;
#pragma unroll
  for (int m = 0; m < 12; ++m) hp[m] = 0.f;
  for (int sgi = 0; sgi < ns; ++sgi, part += kBlockPart) {
#pragma unroll
    for (int m = 0; m < 12; ++m) hp[m] += part[lane + 64 * m];
    if (lane < kBlockWidth) gp += part[768 + lane];
  }
#pragma unroll
  for (int m = 0; m < 12; ++m) block_tile_put(Hs, m >> 2, ((lane + 64 * m) >> 4) & 15, lane & 15, hp[m], reg, bw);
  return gp;
}

// row i of the wave's tile; kPad: a ragged block is padded with the identity here (the implicit row pass adds G[pi_k, pi_k]
// padded that way instead)
template <bool kPad>
__device__ __forceinline__ void block_tile_row(const float* Hs, int i, int bw, float (&hrow)[kBlockWidth]) {
#pragma unroll
  for (int j = 0; j < kBlockWidth; ++j) {
    hrow[j] = Hs[i * kBlockTilePitch + j];
    if constexpr (kPad) hrow[j] = (i >= bw && j == i) ? 1.f : hrow[j];
  }
}

// ---- H d = rhs: lane i (= lane & 31; asm-opaque, see below) holds row i of H in hrow and rhs_i; elimination without pivoting
// (H is symmetric positive definite), pivot row p goes round by readlane; returns d_i
__device__ __forceinline__ float block_solve32(float (&hrow)[kBlockWidth], float rhs, int& i) {
  constexpr int B = kBlockWidth;
  float rd = 0.f;  // lane p: 1 / u_pp
  static_for<B>([&](auto pc) {
    constexpr int p = decltype(pc)::value;
    asm volatile("" : "+v"(i));  // the lane masks of each pivot are compared where they are used, not kept in SGPRs
    const float rinv = 1.f / read_lane(hrow[p], p);
    rd = i == p ? rinv : rd;
    const float l = i > p ? hrow[p] * rinv : 0.f;
    static_for<B>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      if constexpr (j > p) hrow[j] = fmaf(-l, read_lane(hrow[j], p), hrow[j]);
      if constexpr (j > p && (j & 7) == 7) __builtin_amdgcn_sched_barrier(0);  // at most eight pivot-row values in SGPRs
    });
    rhs = fmaf(-l, read_lane(rhs, p), rhs);
  });
  float dv = 0.f;
  static_for<B>([&](auto pc) {
    constexpr int p = B - 1 - decltype(pc)::value;
    asm volatile("" : "+v"(i));
    const float xp = read_lane(rhs * rd, p);
    dv = i == p ? xp : dv;
    rhs = i < p ? fmaf(-hrow[p], xp, rhs) : rhs;
  });
  return dv;
}

// ---- the non-negative block step: z = argmin_{z >= 0} 1/2 z^T H z - c^T z with c = rhs + H x[pi], by block
// principal pivoting (Kim & Park) with Murty's backup rule, the scheme of als_nnls.hip at f = 32 on one wave.  The passive
// set F is a 32-bit mask that every ballot delivers wave-uniform, so the control flow is scalar: no LDS bookkeeping and no
// barrier.  block_solve32 destroys its row, so every step re-reads row i from the wave's tile Hs, which therefore stays live
// until this returns (32 conflict-free LDS reads against an elimination of some 600 VALU instructions; a register copy would
// hold 32 more VGPRs across the solve).  Lanes 32..63 repeat lanes 0..31 throughout; only the low half of a ballot is used.
__device__ __forceinline__ unsigned ballot32(bool p) { return (unsigned)__builtin_amdgcn_ballot_w64(p); }
// the maximum over lanes 0..31 (= over the wave), wave-uniform; fmaxf drops NaN, the callers test finiteness by ballot
__device__ __forceinline__ float block_max32(float v) {
  v = fmaxf(v, dpp_term<0xB1, 0xf>(v));   // quad_perm [1,0,3,2]
  v = fmaxf(v, dpp_term<0x4E, 0xf>(v));   // quad_perm [2,3,0,1]
  v = fmaxf(v, dpp_term<0x141, 0xf>(v));  // row_half_mirror
  v = fmaxf(v, dpp_term<0x140, 0xf>(v));  // row_mirror
  return fmaxf(read_lane(v, 0), read_lane(v, 16));
}
constexpr int kBlockNnlsCap = 16 + 2 * kBlockWidth;  // passive-set steps per block

// Lane i: rhs_i = (g - reg x[pi])_i and the warm start xv = x[pi]_i (both 0 for i >= bw); Hs: the tile, reg on the live
// diagonal.  Returns z_i.  V = {F: z_i < -tol_x} u {G: y_i < -tol}, y = H z - c, tol = 32 2^-24 s, tol_x = tol / max_i H_ii,
// s = max|c| + max_i H_ii max_F|z_i|.  Full exchange while |V| shrinks and three more times after, then Murty's single
// exchange of the largest index.  A step that is not finite, or the cap, ends the block at the last finite iterate clamped
// (none: max(x[pi], 0)) and counts in n_failed; n_elim counts the eliminations.  Padded rows of a ragged block (identity
// diagonal, c = 0) have y = 0: they never enter V and end at 0.
__device__ __forceinline__ float block_nnls32(const float* Hs, int& i, int bw, float rhs, float xv, unsigned& n_failed,
                                              unsigned& n_elim) {
  constexpr int B = kBlockWidth;
  const float* hs = Hs + i * kBlockTilePitch;  // row i of the tile; the identity of the padded rows comes with the mask below
  // the row is read eight elements at a time wherever it is needed: more loads in flight cost registers, not time
  float c = rhs;
  static_for<B>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    c = fmaf(hs[j], read_lane(xv, j), c);
    if constexpr ((j & 7) == 7) __builtin_amdgcn_sched_barrier(0);
  });
  const float max_d = block_max32(i < bw ? hs[i] : 0.f);
  const float max_c = block_max32(fabsf(c));
  const unsigned live = bw < B ? (1u << bw) - 1u : ~0u;
  unsigned F = ballot32(xv > 0.f) & live;
  float zres = fmaxf(xv, 0.f);
  int best = B + 1, backup = 3;
  bool done = false;
  for (int step = 0; step < kBlockNnlsCap; ++step) {
    const bool in_f = (F >> i) & 1u;
    float z = 0.f, y = -c;  // an empty F needs no elimination
    if (F != 0u) {          // uniform
      // the masked system: rows and columns off F (the padded ones are never in F) are the identity, rhs 0 there
      float hrow[B];
      static_for<B>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        hrow[j] = in_f ? ((F >> j) & 1u ? hs[j] : 0.f) : (i == j ? 1.f : 0.f);
        if constexpr ((j & 7) == 7) __builtin_amdgcn_sched_barrier(0);
      });
      z = block_solve32(hrow, in_f ? c : 0.f, i);
      z = in_f ? z : 0.f;
      ++n_elim;
      y = 0.f;
      if (F != live) {  // uniform: a full F has no y
        float hz = 0.f;
        static_for<B>([&](auto jc) {
          constexpr int j = decltype(jc)::value;
          hz = fmaf(hs[j], read_lane(z, j), hz);
          if constexpr ((j & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        });
        y = in_f ? 0.f : hz - c;
      }
    }
    const float s = max_c + max_d * block_max32(fabsf(z));
    const float tol = 0x1p-19f * s;  // 32 2^-24 s
    const float tol_x = max_d > 0.f ? tol / max_d : 0.f;
    if (ballot32(!(isfinite(z) && isfinite(y))) != 0u || !isfinite(tol)) break;
    zres = fmaxf(z, 0.f);
    const unsigned V = ballot32(in_f ? z < -tol_x : y < -tol) & live;
    const int nv = __popc(V);
    if (nv == 0) {
      done = true;
      break;
    }
    unsigned E = V;  // full exchange
    if (nv < best) {
      best = nv;
      backup = 3;
    } else if (backup > 0) {
      --backup;
    } else {  // Murty: the largest infeasible index alone
      E = 1u << (31 - __clz(V));
    }
    F ^= E;
  }
  n_failed += done ? 0u : 1u;
  return zres;
}

}  // namespace cumf

#endif  // CUMF_ALS_BLOCK_CORE_H_
