// als_block.hip -- the kernels of the iALS++ block solver of implicit feedback (als_block.h; CUMF_SOLVER_BLOCK), on the plan's
// segment lists (als_free.h: one wave per segment of at most kFreeSeg entries, so rows of any length work), and the explicit
// block solver's route for rows longer than one segment: block_sparse_kernel at kFreeWeightNone and block_row_free_kernel, the
// row pass without the Gram term; and the weighted block solver's (kFreeWeightArray / kFreeWeightRank1; the row pass with the
// row's scale on the Gram term, over a row list; kNonneg: the 32-wide NNLS in place of the elimination).  The device functions they share with the fused kernels are als_block_core.h.
//   block_open_kernel    one wave per segment: yhat_e = t_e . x (lane l holds features l + 64 q; the transposing wave reduction
//                        of als_device.h);
//   block_sparse_kernel  one wave per segment and block step: the block's 128-byte slice of each gathered row lands directly in
//                        MFMA operand layout -- of four entries at a time, lane i + 16 kappa holds t_kappa[32 k + i] and
//                        t_kappa[32 k + 16 + i], so the 16 lanes of a group read one contiguous 64-byte half-slice and nothing
//                        is transposed through LDS.  Per four entries: yhat += t[pi_prev] . d_prev (16-lane DPP row sum),
//                        c = (1 + w) p - w yhat, g += t c on the VALU and H00 | H01 | H11 += (w t)(t)^T as three
//                        v_mfma_f32_16x16x4_f32 with K over the four entries.  One partial per segment.
//   block_row_kernel     kFreeRows rows per workgroup: x staged in LDS, (G x)[rows, pi_k] on the fp32 matrix pipe (one 16 x 16
//                        tile per wave, K = f, G's 32-column slab read from L2 once per workgroup), then one wave per row: the
//                        segment partials summed in segment order, H01 mirrored, reg and G[pi_k, pi_k] added, a ragged block
//                        padded with the identity, and the 32 x 32 system eliminated without pivoting in registers -- lane i
//                        holds row i, the pivot row goes round by v_readlane -- one system per wave.
// Every sum runs in a fixed order.  No float atomics.
#include <hip/hip_runtime.h>

#include "als_block_core.h"

namespace cumf {

// ---- the opening pass: yhat_e = t_e . x, the T v half of free_sparse_pass
template <int Q>
__global__ __launch_bounds__(kFreeThreads) void block_open_kernel(const BlockArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int f = a.f;
  for (long long sg = (long long)blockIdx.x * 4 + wave; sg < a.nseg; sg += (long long)gridDim.x * 4) {
    const int row = a.seg_row[sg];
    const long long begin = a.seg_begin[sg];
    const int len = a.seg_len[sg];
    float v[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) v[q] = lane + 64 * q < f ? a.x[(size_t)row * f + lane + 64 * q] : 0.f;
    block_open_pass<Q>(a, begin, len, v, lane, [&](int off, float u) { a.yhat[begin + off - a.ent0] = u; });
  }
}

// ---- the block sparse pass of step k.  have_prev: yhat is one block step behind x; the step d of block prev (k - 1, or the
// last block when k = 0) is added first and yhat stored.  kFreeWeightAlpha: the implicit model's confidence weights;
// kFreeWeightNone: the explicit model, w = 1 and c_e = r_e - yhat_e.
template <int B, FreeWeight kWeight>
__global__ __launch_bounds__(kFreeThreads) void block_sparse_kernel(const BlockArgs a, int k, int have_prev) {
  static_assert(B == 32, "two 16-wide half-slices per entry");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, kap = lane >> 4;
  const int f = a.f;
  const BlockCols bc = block_cols(f, k, i);
  for (long long sg = (long long)blockIdx.x * 4 + wave; sg < a.nseg; sg += (long long)gridDim.x * 4) {
    const int row = a.seg_row[sg];
    const long long begin = a.seg_begin[sg];
    const int len = a.seg_len[sg];
    float d0 = 0.f, d1 = 0.f;
    if (have_prev) {
      d0 = a.d[(size_t)row * B + i];
      d1 = a.d[(size_t)row * B + 16 + i];
    }
    [[maybe_unused]] float aw = 0.f;  // kFreeWeightRank1: the row's factor of its unstored weights (uniform)
    if constexpr (kWeight == kFreeWeightRank1) aw = a.own_w0[row];
    BlockAcc acc = block_acc_zero();
    for (int s = 0; s < len; s += 64) {
      const int cnt64 = len - s < 64 ? len - s : 64;
      const bool live = lane < cnt64;
      const long long e = begin + s + lane;
      const int jl = live ? a.colidx[e] : 0;
      const float rl = live ? a.val[e] : 0.f;
      const float yl = live ? a.yhat[e - a.ent0] : 0.f;
      float wl, cl;
      block_entry_weight<kWeight>(a, e, live, jl, rl, aw, wl, cl);
      // lane (kap, i) collects the new yhat of entry 4 i + kap
      const float ynew = block_accumulate64<kWeight>(a.gather, f, bc, cnt64, jl, wl, cl, yl, have_prev, d0, d1, i, kap, acc);
      if (have_prev && 4 * i + kap < cnt64) a.yhat[begin + s + 4 * i + kap - a.ent0] = ynew;
    }
    const float g0 = block_g_sum(acc.g0, i), g1 = block_g_sum(acc.g1, i);
    float* out = a.part + (size_t)sg * kBlockPart;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      out[(4 * kap + r) * 16 + i] = acc.H00[r];
      out[256 + (4 * kap + r) * 16 + i] = acc.H01[r];
      out[512 + (4 * kap + r) * 16 + i] = acc.H11[r];
    }
    if (kap == 0) out[768 + i] = g0, out[768 + 16 + i] = g1;
  }
}

// ---- the block row pass of step k.  first: rows without stored entries get 0 in the block's slice of x and in d.
// rows: NULL for the rows [0, nrows) with their partials at row_seg0, or a list of nrows rows whose partials start at
// pseg0[.] (the long rows of a BlockRowLists).  kScaled (the weighted clients): the Gram term of row u is s_u G, s_u =
// own_w0[u] where that is given, else w0 -- gx and the live part of gpp are multiplied where they are used, as kScale of
// free_gram_rows multiplies G v; the identity that pads a ragged block is not scaled.  Without kScaled the expressions are
// the implicit model's own.
// kNonneg: the block step under x >= 0.  The MFMA phase is the workgroup's last common work: after its barrier every wave owns
// its rows (wave, wave + 4, ..) and its tile hs[wave] and meets no further barrier, so the pivoting loop of block_nnls32, whose
// trip count differs from row to row, holds up only the wave it runs on -- the other three go on through their own rows and
// retire while it pivots; only the workgroup's LDS stays allocated until the last of them ends.  The lanes write the whole
// H = (h + reg) + s_u G[pi_k, pi_k] back into the wave's tile (the sum the elimination takes in registers), block_nnls32 re-reads
// it per passive set, x[pi_k] = z and d = z - x[pi_k].  gx, gpp and vs are read only, so a row's result depends on the row
// alone.  stats as in block_fused_kernel, summed over the wave's rows.
template <int Q, int B, bool kScaled, bool kNonneg>
__global__ __launch_bounds__(kFreeThreads) void block_row_kernel(const BlockArgs a, const int* rows, const int* pseg0,
                                                                 long long nrows, int k, int first,
                                                                 unsigned long long* stats) {
  static_assert(B == 32, "two 16-row tiles x two 16-column tiles, one per wave; one matrix row per lane of a half wave");
  constexpr int P = 64 * Q + 4;  // LDS pitch of the staged x: the 16 rows one MFMA operand reads start 4 banks apart
  constexpr int HP = kBlockTilePitch;
  __shared__ float vs[kFreeRows * P];
  __shared__ float gx[kFreeRows * HP];  // (G x)[rows, pi_k]
  __shared__ float gpp[B * HP];         // G[pi_k, pi_k], a ragged block padded with the identity
  __shared__ float hs[4][B * HP];       // per wave: the row's H
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int f = a.f, KP = (f + 3) & ~3;
  const int c0 = B * k, bw = f - c0 < B ? f - c0 : B;
  const long long r0 = (long long)blockIdx.x * kFreeRows;
  const int nr = (int)(nrows - r0 < kFreeRows ? nrows - r0 : kFreeRows);
  auto row_of = [&](int rr) -> long long { return rows ? (long long)rows[r0 + rr] : r0 + rr; };
  for (int e = threadIdx.x; e < kFreeRows * KP; e += kFreeThreads) {
    const int rr = e / KP, c = e - rr * KP;
    vs[rr * P + c] = (rr < nr && c < f) ? a.x[(size_t)row_of(rr) * f + c] : 0.f;
  }
  for (int e = threadIdx.x; e < B * B; e += kFreeThreads) {
    const int ri = e / B, ci = e - ri * B;
    gpp[ri * HP + ci] = (ri < bw && ci < bw) ? a.G[(size_t)(c0 + ri) * f + c0 + ci] : (ri == ci ? 1.f : 0.f);
  }
  __syncthreads();
  {
    // wave w: rows 16 h .. 16 h + 15, columns 16 J .. 16 J + 15 of the block; A[i][k] = x_i[k] (LDS), B[k][j] = G[k][c0 + 16 J + j]
    // (L2); even and odd K steps in two accumulators, added at the end
    const int h = wave >> 1, J = wave & 1;
    const int col = c0 + 16 * J + (lane & 15);
    const bool colok = col < f;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
    const float* xa = vs + (16 * h + (lane & 15)) * P + (lane >> 4);
    for (int kk = 0; kk < KP / 4; kk += 2) {
      const int k0 = 4 * kk + (lane >> 4), k1 = k0 + 4;
      const float ga = (k0 < f && colok) ? a.G[(size_t)k0 * f + col] : 0.f;
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[4 * kk], ga, acc0, 0, 0, 0);
      if (kk + 1 < KP / 4) {  // uniform
        const float gb = (k1 < f && colok) ? a.G[(size_t)k1 * f + col] : 0.f;
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[4 * kk + 4], gb, acc1, 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) gx[(16 * h + 4 * (lane >> 4) + r) * HP + 16 * J + (lane & 15)] = acc0[r] + acc1[r];
  }
  __syncthreads();
  float* Hs = hs[wave];
  [[maybe_unused]] unsigned n_failed = 0, n_elim = 0;
  for (int rr = wave; rr < nr; rr += 4) {
    int i = lane & 31;  // the matrix row of this lane (the upper half wave repeats the lower and writes nothing)
    const long long row = row_of(rr);
    const int n = a.row_len[row];
    if (n == 0) {  // uniform
      if (first) {
        if (lane < bw) a.x[(size_t)row * f + c0 + lane] = 0.f;
        if (lane < B) a.d[(size_t)row * B + lane] = 0.f;
      }
      continue;
    }
    const float reg = a.reg_mode == kFreeRegPlain ? a.lambda : (float)n * a.lambda;
    // the tiles into the wave's H: the upper triangles of H00 and H11 and all of H01, mirrored
    const int ps0 = rows ? pseg0[r0 + rr] : a.row_seg0[row];
    const float gp = block_partials_to_tile(a.part + (size_t)ps0 * kBlockPart, a.row_nseg[row], Hs, lane, reg, bw);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
    float hrow[B];
    const float xv = i < bw ? vs[rr * P + c0 + i] : 0.f;
    float rhs;
    if constexpr (kScaled) {
      const float su = a.own_w0 ? a.own_w0[row] : a.w0;  // uniform
#pragma unroll
      for (int j = 0; j < B; ++j) hrow[j] = Hs[i * HP + j] + ((i < bw && j < bw) ? su * gpp[i * HP + j] : gpp[i * HP + j]);
      rhs = i < bw ? (gp - su * gx[rr * HP + i]) - reg * xv : 0.f;
    } else {
#pragma unroll
      for (int j = 0; j < B; ++j) hrow[j] = Hs[i * HP + j] + gpp[i * HP + j];
      rhs = i < bw ? (gp - gx[rr * HP + i]) - reg * xv : 0.f;
    }
    if constexpr (kNonneg) {
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      __builtin_amdgcn_wave_barrier();  // both half waves have read row i
      if (lane < B) {
#pragma unroll
        for (int j = 0; j < B; ++j) Hs[i * HP + j] = hrow[j];
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      __builtin_amdgcn_wave_barrier();
      const float z = block_nnls32(Hs, i, bw, rhs, xv, n_failed, n_elim);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      __builtin_amdgcn_wave_barrier();  // Hs is free for the wave's next row
      if (lane < B) {
        if (lane < bw) a.x[(size_t)row * f + c0 + lane] = z;
        a.d[(size_t)row * B + lane] = z - xv;
      }
    } else {
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      __builtin_amdgcn_wave_barrier();  // Hs is free for the wave's next row
      const float dv = block_solve32(hrow, rhs, i);
      if (lane < B) {
        if (lane < bw) a.x[(size_t)row * f + c0 + lane] = xv + dv;
        a.d[(size_t)row * B + lane] = dv;
      }
    }
  }
  if constexpr (kNonneg)
    if (stats && lane == 0) {
      if (n_failed) atomicAdd(stats, (unsigned long long)n_failed);
      if (n_elim) atomicAdd(stats + 1, (unsigned long long)n_elim);
    }
}

// ---- the row pass of the explicit model, whose A = T^T T + reg I has no Gram term: rhs = g - reg x[pi_k], nothing is staged
// and no row needs another, so one wave takes one row of the list `rows` (its partials start at partial pseg0[.]).
// kNonneg: block_nnls32 in place of the elimination, x[pi_k] = z, d = z - x[pi_k]; stats as in block_fused_kernel.
// kRegMode (the weighted client): reg follows a.reg_mode; without it reg = (float)n lambda, the explicit model's.
template <int B, bool kNonneg, bool kRegMode = false>
__global__ __launch_bounds__(kFreeThreads) void block_row_free_kernel(const BlockArgs a, const int* rows, const int* pseg0,
                                                                      long long nrows, int k, int first,
                                                                      unsigned long long* stats) {
  constexpr int HP = kBlockTilePitch;
  __shared__ float hs[4][B * HP];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long idx = (long long)blockIdx.x * 4 + wave;
  if (idx >= nrows) return;  // uniform; the kernel has no workgroup barrier
  const int f = a.f;
  const int c0 = B * k, bw = f - c0 < B ? f - c0 : B;
  float* Hs = hs[wave];
  int i = lane & 31;
  const long long row = rows[idx];
  const int n = a.row_len[row];
  if (n == 0) {  // uniform
    if (first) {
      if (lane < bw) a.x[(size_t)row * f + c0 + lane] = 0.f;
      if (lane < B) a.d[(size_t)row * B + lane] = 0.f;
    }
    return;
  }
  float reg = (float)n * a.lambda;
  if constexpr (kRegMode) reg = a.reg_mode == kFreeRegPlain ? a.lambda : reg;
  const float gp = block_partials_to_tile(a.part + (size_t)pseg0[idx] * kBlockPart, a.row_nseg[row], Hs, lane, reg, bw);
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
  [[maybe_unused]] float hrow[B];
  if constexpr (!kNonneg) block_tile_row<true>(Hs, i, bw, hrow);
  const float xv = i < bw ? a.x[(size_t)row * f + c0 + i] : 0.f;
  const float rhs = i < bw ? gp - reg * xv : 0.f;
  if constexpr (kNonneg) {
    unsigned n_failed = 0, n_elim = 0;
    const float z = block_nnls32(Hs, i, bw, rhs, xv, n_failed, n_elim);
    if (lane < B) {
      if (lane < bw) a.x[(size_t)row * f + c0 + lane] = z;
      a.d[(size_t)row * B + lane] = z - xv;
    }
    if (stats && lane == 0) {
      if (n_failed) atomicAdd(stats, (unsigned long long)n_failed);
      if (n_elim) atomicAdd(stats + 1, (unsigned long long)n_elim);
    }
  } else {
    const float dv = block_solve32(hrow, rhs, i);
    if (lane < B) {
      if (lane < bw) a.x[(size_t)row * f + c0 + lane] = xv + dv;
      a.d[(size_t)row * B + lane] = dv;
    }
  }
}

hipError_t launch_block_open(const BlockArgs& a, hipStream_t stream) {
  if (a.nseg <= 0) return hipSuccess;
  return with_nb<1, 8>((a.f + 63) / 64, [&](auto qc) {
    return launch_kernel(block_open_kernel<decltype(qc)::value>, dim3(free_grid(a.nseg, 4, 16384)), dim3(kFreeThreads), 0,
                         stream, a);
  });
}

hipError_t launch_block_step(const BlockArgs& a, int k, int have_prev, int first, hipStream_t stream) {
  if (a.nseg > 0) {
    const hipError_t e = launch_kernel(block_sparse_kernel<kBlockWidth, kFreeWeightAlpha>, dim3(free_grid(a.nseg, 4, 16384)),
                                       dim3(kFreeThreads), 0, stream, a, k, have_prev);
    if (e != hipSuccess) return e;
  }
  return with_nb<1, 8>((a.f + 63) / 64, [&](auto qc) {
    return launch_item_kernel(block_row_kernel<decltype(qc)::value, kBlockWidth, false, false>,
                              dim3(free_grid(a.rows, kFreeRows, 1ll << 30)), dim3(kFreeThreads), 0, stream, a,
                              (const int*)nullptr, (const int*)nullptr, a.rows, k, first, (unsigned long long*)nullptr);
  });
}

hipError_t launch_block_step_explicit(const BlockArgs& a, const int* rows, const int* pseg0, long long nrows, int k,
                                      int have_prev, int first, bool nonneg, long long* stats, hipStream_t stream) {
  if (nrows <= 0) return hipSuccess;
  if (a.nseg > 0) {
    const hipError_t e = launch_kernel(block_sparse_kernel<kBlockWidth, kFreeWeightNone>, dim3(free_grid(a.nseg, 4, 16384)),
                                       dim3(kFreeThreads), 0, stream, a, k, have_prev);
    if (e != hipSuccess) return e;
  }
  return launch_item_kernel(nonneg ? block_row_free_kernel<kBlockWidth, true> : block_row_free_kernel<kBlockWidth, false>,
                            dim3(free_grid(nrows, 4, 1ll << 30)), dim3(kFreeThreads), 0, stream, a, rows, pseg0, nrows, k, first,
                            reinterpret_cast<unsigned long long*>(stats));
}

hipError_t launch_block_step_weighted(const BlockArgs& a, const int* rows, const int* pseg0, long long nrows, int k,
                                      int have_prev, int first, int mode, bool nonneg, long long* stats, hipStream_t stream) {
  if (nrows <= 0) return hipSuccess;
  auto* st = reinterpret_cast<unsigned long long*>(stats);
  if (a.nseg > 0) {
    const hipError_t e = launch_kernel(mode == kBlockWeightRank1 ? block_sparse_kernel<kBlockWidth, kFreeWeightRank1>
                                                                 : block_sparse_kernel<kBlockWidth, kFreeWeightArray>,
                                       dim3(free_grid(a.nseg, 4, 16384)), dim3(kFreeThreads), 0, stream, a, k, have_prev);
    if (e != hipSuccess) return e;
  }
  if (mode == kBlockWeightPlain)
    return launch_item_kernel(nonneg ? block_row_free_kernel<kBlockWidth, true, true> : block_row_free_kernel<kBlockWidth, false, true>,
                              dim3(free_grid(nrows, 4, 1ll << 30)), dim3(kFreeThreads), 0, stream, a, rows, pseg0, nrows, k, first, st);
  return with_nb<1, 8>((a.f + 63) / 64, [&](auto qc) {
    constexpr int Q = decltype(qc)::value;
    return launch_item_kernel(nonneg ? block_row_kernel<Q, kBlockWidth, true, true> : block_row_kernel<Q, kBlockWidth, true, false>,
                              dim3(free_grid(nrows, kFreeRows, 1ll << 30)), dim3(kFreeThreads), 0, stream, a, rows, pseg0, nrows,
                              k, first, st);
  });
}

}  // namespace cumf
