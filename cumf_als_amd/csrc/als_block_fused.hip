// als_block_fused.hip -- the fused kernel of the explicit block solver (als_block.h: update_block_explicit): one wave runs the
// whole half-iteration of one row of at most `cap` <= kFreeSeg stored entries -- the opening pass, every sweep, every block --
// in one launch.  The explicit A = T^T T + reg I has no Gram term, so a block step needs nothing from another row.
//   yhat   one float per stored entry in the wave's LDS slice, one block step behind x exactly as on the segmented route;
//   x      in registers in the opening pass's layout (lane l holds features l + 64 q).  Block k is lanes 32 (k & 1) .. of
//          register k >> 1 and the solve leaves d in lanes 0..31 repeated in lanes 32..63, so x[pi_k] += d is one masked add
//          per register with no shuffle and no LDS: nothing to size, no ordering to keep, and the final store is the coalesced
//          row store of the opening layout.  x is written to global memory once, at the end;
//   d      stays in registers between the solve and the next block's accumulate (two ds_bpermute into the MFMA layout);
//   H, g   the accumulators of als_block_core.h, scattered straight from the MFMA layout into the wave's 32 x 33 LDS tile.
// Every value is formed by the functions of als_block_core.h from the same terms in the same order as block_open_kernel,
// block_sparse_kernel<32, kFreeWeightNone> and block_row_free_kernel form it: a row's bits do not depend on the route.
// LDS per wave: 4 B x cap + 4 224 B, dynamic, so one instance per Q = ceil(f / 64) serves every capacity class.
#include <hip/hip_runtime.h>

#include "als_block_core.h"

namespace cumf {

// kNonneg: the block step is block_nnls32 on the same tile and right-hand side, x[pi_k] = z and d = z - x[pi_k]; the tile stays
// live through it.  stats (kNonneg only, may be NULL): (blocks not converged, eliminations), summed per wave, integer atomics.
// kWeight: kFreeWeightNone, the explicit model, or kFreeWeightArray, the weighted model without a Gram term (w0 == 0: the
// entry's weight is one more coalesced load per 64 entries, and reg follows a.reg_mode).
template <int Q, bool kNonneg, FreeWeight kWeight>
__global__ __launch_bounds__(kFreeThreads) void block_fused_kernel(const BlockArgs a, const int* rows, long long nrows, int cap,
                                                                   int sweeps, unsigned long long* stats) {
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
  float reg = (float)n * a.lambda;
  if constexpr (kWeight != kFreeWeightNone) reg = a.reg_mode == kFreeRegPlain ? a.lambda : reg;
  float v[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) v[q] = lane + 64 * q < f ? xrow[lane + 64 * q] : 0.f;
  block_open_pass<Q>(a, begin, n, v, lane, [&](int off, float u) { ys[off] = u; });
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
        block_entry_weight<kWeight>(a, begin + s + lane, live, jl, rl, 0.f, wl, cl);
        const float ynew = block_accumulate64<kWeight>(a.gather, f, bc, cnt64, jl, wl, cl, yl, have_prev, d0, d1, i16, kap, acc);
        if (have_prev && 4 * i16 + kap < cnt64) ys[s + 4 * i16 + kap] = ynew;
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
      [[maybe_unused]] float hrow[B];
      if constexpr (!kNonneg) block_tile_row<true>(Hs, i, bw, hrow);
      // x[pi_k]: register k >> 1, lanes 32 (k & 1) ..; the solve wants feature c0 + i in lane i of both halves
      float xk = 0.f;
#pragma unroll
      for (int q = 0; q < Q; ++q) xk = q == (k >> 1) ? v[q] : xk;
      const float xs = __shfl(xk, 32 * (k & 1) + i);
      const float xv = i < bw ? xs : 0.f;
      const float gp = i < 16 ? g0 : g1;  // g[i]: lane groups 1 and 3 hold g[16 + i16] in g1
      const float rhs = i < bw ? gp - reg * xv : 0.f;
      [[maybe_unused]] float z = 0.f;
      if constexpr (kNonneg) z = block_nnls32(Hs, i, bw, rhs, xv, n_failed, n_elim);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      __builtin_amdgcn_wave_barrier();  // Hs is free for the next block
      if constexpr (kNonneg) dv = z - xv;
      else dv = block_solve32(hrow, rhs, i);
      const bool mine = (lane >> 5) == (k & 1) && i < bw;
#pragma unroll
      for (int q = 0; q < Q; ++q) v[q] = (mine && q == (k >> 1)) ? (kNonneg ? z : v[q] + dv) : v[q];
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

hipError_t launch_block_fused(const BlockArgs& a, const int* rows, long long nrows, int cap, int sweeps, bool nonneg,
                              long long* stats, hipStream_t stream) {
  if (nrows <= 0) return hipSuccess;
  const size_t lds = 4 * (size_t)(kBlockWidth * kBlockTilePitch + cap) * sizeof(float);
  auto* st = reinterpret_cast<unsigned long long*>(stats);
  return with_nb<1, 8>((a.f + 63) / 64, [&](auto qc) {
    constexpr int Q = decltype(qc)::value;
    return launch_item_kernel(nonneg ? block_fused_kernel<Q, true, kFreeWeightNone> : block_fused_kernel<Q, false, kFreeWeightNone>,
                              dim3(free_grid(nrows, 4, 1ll << 30)), dim3(kFreeThreads), lds, stream, a, rows, nrows, cap, sweeps, st);
  });
}

hipError_t launch_block_fused_weighted(const BlockArgs& a, const int* rows, long long nrows, int cap, int sweeps, bool nonneg,
                                       long long* stats, hipStream_t stream) {
  if (nrows <= 0) return hipSuccess;
  const size_t lds = 4 * (size_t)(kBlockWidth * kBlockTilePitch + cap) * sizeof(float);
  auto* st = reinterpret_cast<unsigned long long*>(stats);
  return with_nb<1, 8>((a.f + 63) / 64, [&](auto qc) {
    constexpr int Q = decltype(qc)::value;
    return launch_item_kernel(nonneg ? block_fused_kernel<Q, true, kFreeWeightArray> : block_fused_kernel<Q, false, kFreeWeightArray>,
                              dim3(free_grid(nrows, 4, 1ll << 30)), dim3(kFreeThreads), lds, stream, a, rows, nrows, cap, sweeps, st);
  });
}

}  // namespace cumf
