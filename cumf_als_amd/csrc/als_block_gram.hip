// als_block_gram.hip -- the fused kernel of the weighted block solver for rows whose system carries a Gram term (als_block.h:
// update_block_weighted; A_u = s_u G + sum_e q_e t_e t_e^T + reg I): one wave runs the whole half-iteration of one row of at
// most `cap` <= kFreeSeg stored entries in one launch, as block_fused_kernel (als_block_fused.hip) does for systems without G.
// What that kernel keeps on chip stays there -- yhat in the wave's LDS slice, x in registers in the opening layout (lane l
// holds features l + 64 q), d in registers, the 32 x 33 tile in LDS, no workgroup barrier -- and the Gram term adds
//   u = G x   in registers in the layout of x (Q more VGPRs), independent of the row's scale s_u.  It opens as the chain
//             u[l + 64 q] = fma(G[j f + l + 64 q], x_j, u) over all columns j in increasing order, x_j by v_readlane, and
//             after every block step takes the step the same way: u = fma(G[(c0 + j) f + .], d_j, u), j = 0 .. bw - 1.  Every
//             load is a coalesced row read of G, which is at most 1 MB and stays in L2; (1 + sweeps) f^2 floats per row.
//             (G x)[pi_k] for the right-hand side comes out of register k >> 1 by the shuffle that fetches x[pi_k];
//   s_u G[pi_k, pi_k]  sixteen coalesced loads per lane (two 128-byte rows of the block per instruction), issued after the
//             sparse pass while the tile is written, and added to the tile element by element before lane i reads row i:
//             (h + reg) + s_u G, the sum block_row_kernel forms; a ragged block is padded with the identity (not scaled).
// The sparse terms are formed by als_block_core.h exactly as on the segmented route; (G x) is summed column by column here
// and on the matrix pipe there, so the two routes differ in the last bits.  A row's result depends on the row alone.
// LDS per wave: 4 B x cap + 4 224 B, dynamic: one instance per Q = ceil(f / 64) and weight mode serves every capacity class.
#include <hip/hip_runtime.h>

#include "als_block_core.h"

namespace cumf {

// u[q] = fma(G[(j0 + t) f + lane + 64 q], src_t, u[q]) for t = 0 .. cnt - 1 in increasing t; src_t is lane t of `src`.  N rows
// of G are in flight at a time (N Q loads per lane).
template <int Q>
__device__ __forceinline__ void block_gram_axpy(const float* G, int f, int j0, int cnt, float src, int lane, float (&u)[Q]) {
  constexpr int N = Q <= 2 ? 8 : Q <= 4 ? 4 : 2;
  for (int t0 = 0; t0 < cnt; t0 += N) {
    float g[N][Q];
    static_for<N>([&](auto tc) {
      constexpr int t = decltype(tc)::value;
      const float* row = G + (size_t)(j0 + t0 + t) * f;
#pragma unroll
      for (int q = 0; q < Q; ++q) g[t][q] = (t0 + t < cnt && lane + 64 * q < f) ? row[lane + 64 * q] : 0.f;
    });
    static_for<N>([&](auto tc) {
      constexpr int t = decltype(tc)::value;
      if (t0 + t < cnt) {  // uniform
        const float st = read_lane(src, t0 + t);
#pragma unroll
        for (int q = 0; q < Q; ++q) u[q] = fmaf(g[t][q], st, u[q]);
      }
    });
  }
}

// kWeight: kFreeWeightArray (s_u = a.w0) or kFreeWeightRank1 (s_u = a.own_w0[row])
// kNonneg: the block step under x >= 0.  The tile already holds the whole H = (h + reg) + s_u G[pi_k, pi_k], so block_nnls32
// runs on it as it does in block_fused_kernel: c = rhs + H x[pi_k] from the lane's tile row and the x[pi_k] the shuffle below
// fetched, the passive set in SGPRs, every masked system re-read from the tile, which therefore stays live through the step
// (no row copy in registers: hrow is not loaded).  x[pi_k] = z, d = z - x[pi_k]; u += G[:, pi_k] d and the deferred
// yhat += t[pi_k] . d then run on that d as on the unconstrained one.  stats as in block_fused_kernel.
template <int Q, FreeWeight kWeight, bool kNonneg>
__global__ __launch_bounds__(kFreeThreads) void block_fused_gram_kernel(const BlockArgs a, const int* rows, long long nrows,
                                                                        int cap, int sweeps, unsigned long long* stats) {
  static_assert(kWeight == kFreeWeightArray || kWeight == kFreeWeightRank1, "the weighted clients");
  constexpr int B = kBlockWidth, HP = kBlockTilePitch;
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long idx = (long long)blockIdx.x * 4 + wave;
  if (idx >= nrows) return;  // uniform; the kernel has no workgroup barrier
  float* Hs = lds + (size_t)wave * (B * HP + cap);
  float* ys = Hs + B * HP;
  const int i16 = lane & 15, kap = lane >> 4;
  int i = lane & 31;  // the matrix row of this lane in the solve
  const int f = a.f, nb = (f + B - 1) / B;
  const long long row = rows[idx];
  const int n = a.row_len[row];
  float* xrow = a.x + (size_t)row * f;
  if (n == 0) {  // uniform: no stored entry, x = 0
#pragma unroll
    for (int q = 0; q < Q; ++q)
      if (lane + 64 * q < f) xrow[lane + 64 * q] = 0.f;
    return;
  }
  const long long begin = a.seg_begin[a.row_seg0[row]];
  const float reg = a.reg_mode == kFreeRegPlain ? a.lambda : (float)n * a.lambda;
  float su = a.w0, aw = 0.f;  // uniform: the scale of the row's Gram term, and the row's factor in q_e
  if constexpr (kWeight == kFreeWeightRank1) su = aw = a.own_w0[row];
  float v[Q], u[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) v[q] = lane + 64 * q < f ? xrow[lane + 64 * q] : 0.f, u[q] = 0.f;
  block_open_pass<Q>(a, begin, n, v, lane, [&](int off, float y) { ys[off] = y; });
  // u = G x: column j of x is lane j & 63 of register j >> 6
  static_for<Q>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    const int cnt = f - 64 * q < 64 ? f - 64 * q : 64;
    block_gram_axpy<Q>(a.G, f, 64 * q, cnt, v[q], lane, u);
  });
  float dv = 0.f;  // lanes 0..31 and again 32..63: the step of the block solved last
  [[maybe_unused]] unsigned n_failed = 0, n_elim = 0;
  for (int sweep = 0; sweep < sweeps; ++sweep)
    for (int k = 0; k < nb; ++k) {
      const int have_prev = sweep > 0 || k > 0;
      const int c0 = B * k, bw = f - c0 < B ? f - c0 : B;
      const BlockCols bc = block_cols(f, k, i16);
      const float d0 = __shfl(dv, i16), d1 = __shfl(dv, 16 + i16);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      __builtin_amdgcn_wave_barrier();  // the yhat of the step (or the opening pass) before is in LDS
      BlockAcc acc = block_acc_zero();
      for (int s = 0; s < n; s += 64) {
        const int cnt64 = n - s < 64 ? n - s : 64;
        const bool live = lane < cnt64;
        const int jl = live ? a.colidx[begin + s + lane] : 0;
        const float rl = live ? a.val[begin + s + lane] : 0.f;
        const float yl = live ? ys[s + lane] : 0.f;
        float wl, cl;
        block_entry_weight<kWeight>(a, begin + s + lane, live, jl, rl, aw, wl, cl);
        const float ynew = block_accumulate64<kWeight>(a.gather, f, bc, cnt64, jl, wl, cl, yl, have_prev, d0, d1, i16, kap, acc);
        if (have_prev && 4 * i16 + kap < cnt64) ys[s + 4 * i16 + kap] = ynew;
      }
      // element lane + 64 m of s_u G[pi_k, pi_k], row-major 32 x 32; the loads fly while the tile is written.  Beyond bw the identity, as block_row_kernel pads gpp
      float gpp[B / 2];
#pragma unroll
      for (int m = 0; m < B / 2; ++m) {
        const int ri = 2 * m + (lane >> 5);
        gpp[m] = (ri < bw && i < bw) ? su * a.G[(size_t)(c0 + ri) * f + c0 + i] : (ri == i ? 1.f : 0.f);
      }
      const float g0 = block_g_sum(acc.g0, i16), g1 = block_g_sum(acc.g1, i16);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        block_tile_put(Hs, 0, 4 * kap + r, i16, acc.H00[r], reg, bw);
        block_tile_put(Hs, 1, 4 * kap + r, i16, acc.H01[r], reg, bw);
        block_tile_put(Hs, 2, 4 * kap + r, i16, acc.H11[r], reg, bw);
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int m = 0; m < B / 2; ++m) Hs[(2 * m + (lane >> 5)) * HP + i] += gpp[m];
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      __builtin_amdgcn_wave_barrier();
      [[maybe_unused]] float hrow[B];
      if constexpr (!kNonneg) block_tile_row<false>(Hs, i, bw, hrow);
      // x[pi_k] and (G x)[pi_k]: register k >> 1, lanes 32 (k & 1) ..; the solve wants feature c0 + i in lane i of both halves
      float xk = 0.f, uk = 0.f;
#pragma unroll
      for (int q = 0; q < Q; ++q) xk = q == (k >> 1) ? v[q] : xk, uk = q == (k >> 1) ? u[q] : uk;
      const float xs = __shfl(xk, 32 * (k & 1) + i), us = __shfl(uk, 32 * (k & 1) + i);
      const float xv = i < bw ? xs : 0.f;
      const float gp = i < 16 ? g0 : g1;  // g[i]: lane groups 1 and 3 hold g[16 + i16] in g1
      const float rhs = i < bw ? (gp - su * us) - reg * xv : 0.f;
      [[maybe_unused]] float z = 0.f;
      if constexpr (kNonneg) z = block_nnls32(Hs, i, bw, rhs, xv, n_failed, n_elim);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      __builtin_amdgcn_wave_barrier();  // Hs is free for the next block
      if constexpr (kNonneg) dv = z - xv;
      else dv = block_solve32(hrow, rhs, i);
      const bool mine = (lane >> 5) == (k & 1) && i < bw;
#pragma unroll
      for (int q = 0; q < Q; ++q) v[q] = (mine && q == (k >> 1)) ? (kNonneg ? z : v[q] + dv) : v[q];
      // u += G[:, pi_k] d (G is symmetric: rows c0 .. c0 + bw - 1); nothing reads u after the very last step
      if (sweep + 1 < sweeps || k + 1 < nb) block_gram_axpy<Q>(a.G, f, c0, bw, dv, lane, u);
    }
#pragma unroll
  for (int q = 0; q < Q; ++q)
    if (lane + 64 * q < f) xrow[lane + 64 * q] = v[q];
  if constexpr (kNonneg)
    if (stats && lane == 0) {
      if (n_failed) atomicAdd(stats, (unsigned long long)n_failed);
      if (n_elim) atomicAdd(stats + 1, (unsigned long long)n_elim);
    }
}

hipError_t launch_block_fused_gram(const BlockArgs& a, const int* rows, long long nrows, int cap, int sweeps, int mode,
                                   bool nonneg, long long* stats, hipStream_t stream) {
  if (nrows <= 0) return hipSuccess;
  const size_t lds = 4 * (size_t)(kBlockWidth * kBlockTilePitch + cap) * sizeof(float);
  auto* st = reinterpret_cast<unsigned long long*>(stats);
  return with_nb<1, 8>((a.f + 63) / 64, [&](auto qc) {
    constexpr int Q = decltype(qc)::value;
    auto go = [&](auto kernel) {
      return launch_item_kernel(kernel, dim3(free_grid(nrows, 4, 1ll << 30)), dim3(kFreeThreads), lds, stream, a, rows, nrows,
                                cap, sweeps, st);
    };
    if (mode == kBlockWeightRank1)
      return nonneg ? go(block_fused_gram_kernel<Q, kFreeWeightRank1, true>) : go(block_fused_gram_kernel<Q, kFreeWeightRank1, false>);
    return nonneg ? go(block_fused_gram_kernel<Q, kFreeWeightArray, true>) : go(block_fused_gram_kernel<Q, kFreeWeightArray, false>);
  });
}

}  // namespace cumf
