// als_kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the ALS solve path.
//
// What the reference does per half-iteration (als.cu:727-964):
//   b   = R * Theta            cusparseScsrmm2 + cublasSgeam   (als.cu:750-757)
//   A_u = sum theta theta^T + lambda n_u I   get_hermitian100 / get_hermitianT10
//                                            (als.cu:443-569 / 575-659), one CUDA
//                                            block per row, 10x10 register tiles
//   x_u = A_u^-1 b_u           updateXWithCGKernel (cg.cu:36-231) or cuBLAS batched LU
// with the f x f Gram batch written to and re-read from device memory.
//
// What this file does instead (MI355X-first):
//   * one pass gathers each factor row ONCE into LDS (16-byte loads, zero padded
//     to 16-wide feature blocks, the rating value parked in feature slot f);
//   * the rank-k update theta theta^T is a SYRK on the fp32 matrix cores:
//     v_mfma_f32_16x16x4_f32 over the upper-triangular 16x16 tiles only.  One VGPR
//     per (feature block, 4 ratings) is both the A and the B operand.  The RHS
//     b = sum r theta falls out of column f of the last tile column for free;
//   * rows are cut into chunks (plan, als_plan.cpp) so heavy rows spread over
//     many workgroups; whole rows are solved in the same workgroup straight out of
//     LDS (CG or unpivoted LU) -- the Gram never touches HBM; chunked rows go
//     through a deterministic partial-tile reduction kernel;
//   * fp32 MFMA is an exact k-ordered fmaf chain, so a whole-row Gram entry is the
//     same sequential FMA chain one reference thread computes (als.h:39-143).
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "als_internal.h"
#include "als_device.h"
#include "als_lu_reg.h"
#include "als_lu_wg.h"

namespace cumf {

// The file is compiled once per NB (Makefile: -DCUMF_NB_SLICE=1..13, the kernels of that feature-block count; 0: the
// oracle-order LU alone), so that the build runs in parallel.  Each object instantiates the entry points of its NB only
// (end of file).
#ifndef CUMF_NB_SLICE
#error "compile with -DCUMF_NB_SLICE=<feature blocks>"
#endif

// The accumulator LU pays off from f = 96 on (measured: f = 64 18.8 vs 18.0 ms, f = 10 0.67 vs 0.56 ms with
// the thread-grid LU; f = 100 35.7 vs 36.8, f = 128 62.2 vs 63.8, f = 200 200 vs 224).
constexpr bool lu_on_accumulators(int nb) { return nb >= 7; }



// ----------------------------------------------------------------------------------
// Geometry of one workgroup (256 threads = 4 waves) for NB 16-wide feature blocks.
// ----------------------------------------------------------------------------------
template <int NB>
struct Geo {
  static constexpr int NT = NB * (NB + 1) / 2;  // upper-triangular tiles
  static constexpr int TPW = (NT + 3) / 4;      // tiles per wave (T-split over the 4 waves)
  // Stage row pitch in floats.  LD % 32 == 16 makes the MFMA operand read
  // (lane = 16*kk + c reads stage[4g+kk][16B+c]) conflict-free for ds_read_b32,
  // whose lane groups are {0-31},{32-63} over 32 banks.
  static constexpr int LD = 16 * NB + ((NB % 2 == 0) ? 16 : 0);
  // Tile held in accumulator slot s of wave role W.  Round-robin: every role keeps a similar
  // share of live tiles all through the elimination of lu_solve_mfma (with contiguous ranges the
  // last role owns the tiles that stay live to the end); the price is that every role reads all
  // NB feature blocks in the Gram pass.
  __host__ __device__ static constexpr int tile(int W, int s) {
    return NB >= 7 ? W + 4 * s : W * TPW + s;
  }
};

// ----------------------------------------------------------------------------------
// Global -> register -> LDS staging of kStage gathered factor rows.
// VT is float4 when f % 4 == 0 (16-byte loads; f = 100: 25 loads per row) else float2
// (f % 10 == 0 guarantees f even, main.cpp:33).
// ----------------------------------------------------------------------------------
template <int NB, typename VT>
struct Stager {
  static constexpr int VW = sizeof(VT) / 4;
  static constexpr int LD = Geo<NB>::LD;
  static constexpr int PPR = LD / VW;                 // vector pieces per stage row
  static constexpr int LPR = PPR <= 32 ? 32 : (PPR <= 64 ? 64 : 128);  // lanes covering one row (power of two)
  static constexpr int RPP = kThreads / LPR;          // rows per pass
  static constexpr int PASSES = kStage / RPP;
  static_assert(PPR <= 128, "stage row too wide");
  VT v[PASSES];        // gathered factor-row pieces of one stage
  float rvv;           // rating of row (tid & 31) of that stage
  int cols[PASSES];    // column indices feeding the next gather
  int cols_nx[PASSES]; // column indices one stage further ahead
  // loop-invariant per-thread state
  unsigned goff;       // byte offset of this lane's piece inside a factor row (clamped)
  int lds_row0;        // float offset of (row rsub, this piece) inside a stage buffer
  bool feat;           // this lane's piece holds features (col0 < f)
  int rsub, col0;

  // The steady-state stage loop must stay ONE basic block with as few VALU instructions as
  // possible: measured with tools/probes/mfma_ladder.hip, every VALU instruction issued next to the
  // MFMAs costs matrix-pipe time, and a load under a branch degrades every s_waitcnt to
  // vmcnt(0).  So: full stages take a select-free path (feature lanes store what they loaded,
  // the zero padding of the stage rows is written once per item, the rating goes through its
  // own 4-byte store), addresses are 32-bit offsets from wave-uniform bases (factor tables
  // are < 4 GiB), and only the last -- possibly ragged -- stage of an item uses masked stores.
  __device__ __forceinline__ void init(int f, int tid) {
    const int pc = tid % LPR;
    rsub = tid / LPR;
    col0 = pc * VW;
    feat = col0 < f;
    goff = feat ? (unsigned)col0 * 4u : 0u;
    lds_row0 = rsub * LD + col0;
  }

  // Zero the padding of both stage buffers: columns [f + VW, LD) of every row (the piece at
  // column f carries the rating and is rewritten whole per stage).  Needed once per item (the
  // solvers' G aliases the buffers).
  __device__ __forceinline__ void zero_padding(float* __restrict__ smem, int f, int tid) const {
    const int pieces = (LD - f) / VW - 1;  // per row
    for (int e = tid; e < 2 * kStage * pieces; e += kThreads) {
      const int row = e / pieces, k = e - row * pieces;
      VT z = {};
      *reinterpret_cast<VT*>(smem + row * LD + f + (k + 1) * VW) = z;
    }
  }

  template <bool FULL>
  __device__ __forceinline__ void load_cols_into(int (&dst)[PASSES], const int* __restrict__ colidx, long long begin,
                                                 int nvalid) {
    const int* base = colidx + begin;  // wave-uniform
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int r = rsub + p * RPP;
      dst[p] = base[(unsigned)(FULL ? r : (r < nvalid ? r : nvalid - 1))];
    }
  }

  // Gather of one stage: pass p loads VW consecutive features of factor row cols[p]; the
  // rating of row (tid & 31) rides along.  Nothing here consumes a loaded value.
  template <int P>
  __device__ __forceinline__ void gather_pass(const float* __restrict__ gat, unsigned f4) {
    const unsigned off = (unsigned)cols[P] * f4 + goff;  // bytes, < 4 GiB
    v[P] = *reinterpret_cast<const VT*>(reinterpret_cast<const char*>(gat) + off);
  }
  template <bool FULL>
  __device__ __forceinline__ void gather_val(const float* __restrict__ val, long long begin, int nvalid, int tid) {
    const int r = tid & (kStage - 1);
    if (val == nullptr) {  // no ratings given (alsUpdateFeature100Host: the right-hand side comes precomputed): zeros
      rvv = 0.f;
      return;
    }
    const float* vbase = val + begin;  // wave-uniform
    rvv = vbase[(unsigned)(FULL ? r : (r < nvalid ? r : nvalid - 1))];
  }
  template <bool FULL>
  __device__ __forceinline__ void gather(const float* __restrict__ val, const float* __restrict__ gat, unsigned f4,
                                         long long begin, int nvalid, int tid) {
    static_for<PASSES>([&](auto pc) { gather_pass<decltype(pc)::value>(gat, f4); });
    gather_val<FULL>(val, begin, nvalid, tid);
  }

  // Full stage: feature lanes store their piece as loaded; other lanes hit the dummy slot.
  template <int P>
  __device__ __forceinline__ void store_pass_full(float* __restrict__ stage, float* __restrict__ dummy) const {
    float* dst = feat ? stage + lds_row0 + P * RPP * LD : dummy;
    *reinterpret_cast<VT*>(dst) = v[P];
  }
  __device__ __forceinline__ void store_val_full(float* __restrict__ stage, int f, int tid) const {
    VT x = {};
    x[0] = rvv;  // the whole piece {rating, 0, ...}; 8 threads per row write the same value
    *reinterpret_cast<VT*>(stage + (tid & (kStage - 1)) * LD + f) = x;
  }
  // Ragged stage: rows [nvalid, nwrite) are written as zeros (nwrite = nvalid rounded up to 4).
  template <int P>
  __device__ __forceinline__ void store_pass_masked(float* __restrict__ stage, float* __restrict__ dummy, int nvalid,
                                                    int nwrite) const {
    const int r = rsub + P * RPP;
    VT x = v[P];
#pragma unroll
    for (int e = 0; e < VW; ++e) x[e] = (r < nvalid) ? x[e] : 0.f;
    float* dst = (feat && r < nwrite) ? stage + lds_row0 + P * RPP * LD : dummy;
    *reinterpret_cast<VT*>(dst) = x;
  }
  __device__ __forceinline__ void store_val_masked(float* __restrict__ stage, float* __restrict__ dummy, int f,
                                                   int nvalid, int nwrite, int tid) const {
    const int r = tid & (kStage - 1);
    float* dst = (r < nwrite) ? stage + r * LD + f : dummy;
    VT x = {};
    x[0] = (r < nvalid) ? rvv : 0.f;
    *reinterpret_cast<VT*>(dst) = x;
  }
  __device__ __forceinline__ void store_masked(float* __restrict__ stage, float* __restrict__ dummy, int f, int nvalid,
                                               int nwrite, int tid) const {
    static_for<PASSES>([&](auto pc) { store_pass_masked<decltype(pc)::value>(stage, dummy, nvalid, nwrite); });
    store_val_masked(stage, dummy, f, nvalid, nwrite, tid);
  }
  __device__ __forceinline__ void rotate_cols() {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) cols[p] = cols_nx[p];
  }
};

// ----------------------------------------------------------------------------------
// SYRK of one stage on the matrix cores.  Wave W owns tiles [W*TPW, (W+1)*TPW).
//   D[i][j] += sum_k A[i][k] B[k][j],  A[i][k] = theta_k[16I+i], B[k][j] = theta_k[16J+j]
// v_mfma_f32_16x16x4_f32 operand layout: lane l supplies A[l&15][l>>4] and
// B[l>>4][l&15]; both are stage[4g + (l>>4)][16*blk + (l&15)], so a feature
// block's register serves as the A operand of its tile row and the B operand of its
// tile column.  Accumulation is the exact k-ordered fmaf chain (rating order).
// ----------------------------------------------------------------------------------
template <int NB, int W>
__device__ __forceinline__ void mma_group(const float (&blk)[NB], f32x4 (&acc)[Geo<NB>::TPW]) {
  constexpr int NT = Geo<NB>::NT, TPW = Geo<NB>::TPW;
  static_for<TPW>([&](auto sc) {
    constexpr int s = decltype(sc)::value;
    constexpr int t = Geo<NB>::tile(W, s);
    if constexpr (t < NT) {
      constexpr int I = tile_I<NB>(t), J = tile_J<NB>(t);
      acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(blk[I], blk[J], acc[s], 0, 0, 0);
    }
  });
}

template <int NB, int W>
__device__ __forceinline__ void mma_stage(const float* __restrict__ stage, f32x4 (&acc)[Geo<NB>::TPW],
                                          int ngroups, int lane) {
  constexpr int LD = Geo<NB>::LD;
  const float* rowp = stage + (lane >> 4) * LD + (lane & 15);
  // Software-pipelined by hand: the operand reads of group g+1 are issued before the MFMAs
  // of group g so that LDS latency hides behind the matrix pipe (the scheduler sinks the
  // reads next to their use otherwise, hence the sched_barriers).  Blocks this wave never
  // uses are dead code.  The read-ahead may run up to two groups past `ngroups`: it stays
  // inside the LDS allocation (launch_nb pads it) and the values are never used.
  auto load_blk = [&](float (&blk)[NB], const float* p) {
#pragma unroll
    for (int b = 0; b < NB; ++b) blk[b] = p[16 * b];
  };
  float blk_a[NB], blk_b[NB];
  load_blk(blk_a, rowp);
  int g = 0;
  for (; g + 1 < ngroups; g += 2) {
    load_blk(blk_b, rowp + 4 * LD);
    __builtin_amdgcn_sched_barrier(0);
    mma_group<NB, W>(blk_a, acc);
    __builtin_amdgcn_sched_barrier(0);
    load_blk(blk_a, rowp + 8 * LD);
    __builtin_amdgcn_sched_barrier(0);
    mma_group<NB, W>(blk_b, acc);
    __builtin_amdgcn_sched_barrier(0);
    rowp += 8 * LD;
  }
  if (g < ngroups) mma_group<NB, W>(blk_a, acc);
}

// Accumulator tiles -> LDS, tile-major ([tile][16][16], rows permuted by tiled_row): the
// hand-over to lu_solve_reg, whose threads pick their elements up with TileLoad.
template <int NB, int W>
__device__ __forceinline__ void tiles_to_tiled(const f32x4 (&acc)[Geo<NB>::TPW], float* __restrict__ T,
                                               float reg, int lane) {
  constexpr int NT = Geo<NB>::NT, TPW = Geo<NB>::TPW;
  const int c = lane & 15, kk = lane >> 4;
  static_for<TPW>([&](auto sc) {
    constexpr int s = decltype(sc)::value;
    constexpr int t = Geo<NB>::tile(W, s);
    if constexpr (t < NT) {
      constexpr int I = tile_I<NB>(t), J = tile_J<NB>(t);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[s][r];
        if (I == J && 4 * kk + r == c) v += reg;  // lambda * n_u on the diagonal (als.cu:545-557)
        T[256 * t + (4 * r + kk) * 16 + c] = v;
      }
    }
  });
}

// Accumulator tile -> LDS system matrix G (f x ldg, column f = RHS).  C/D layout of
// the 16x16 MFMA: lane l, register r holds D[4*(l>>4) + r][l & 15].
template <int NB, int W>
__device__ __forceinline__ void tiles_to_lds(const f32x4 (&acc)[Geo<NB>::TPW], float* __restrict__ G,
                                             int ldg, int f, float reg, int lane) {
  constexpr int NT = Geo<NB>::NT, TPW = Geo<NB>::TPW;
  const int c = lane & 15, kk = lane >> 4;
  static_for<TPW>([&](auto sc) {
    constexpr int s = decltype(sc)::value;
    constexpr int t = Geo<NB>::tile(W, s);
    if constexpr (t < NT) {
      constexpr int I = tile_I<NB>(t), J = tile_J<NB>(t);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * I + 4 * kk + r, j = 16 * J + c;
        float v = acc[s][r];
        if (I == J && i == j) v += reg;                    // lambda * n_u on the diagonal (als.cu:545-557)
        if (i < f && j <= f) G[i * ldg + j] = v;           // j == f: b_i = sum r * theta[i]
        if (I != J && i < f && j < f) G[j * ldg + i] = v;  // mirror
      }
    }
  });
}

// Accumulator tile -> row-major f x f Gram in global memory (both triangles,
// lambda * n on the diagonal: als.cu:545-566) + RHS.
template <int NB, int W, typename T>
__device__ __forceinline__ void tiles_to_global(const f32x4 (&acc)[Geo<NB>::TPW], T* __restrict__ tt,
                                                float* __restrict__ rhs, int f, float reg, int lane,
                                                bool packed = false) {
  constexpr int NT = Geo<NB>::NT, TPW = Geo<NB>::TPW;
  const int c = lane & 15, kk = lane >> 4;
  static_for<TPW>([&](auto sc) {
    constexpr int s = decltype(sc)::value;
    constexpr int t = Geo<NB>::tile(W, s);
    if constexpr (t < NT) {
      constexpr int I = tile_I<NB>(t), J = tile_J<NB>(t);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * I + 4 * kk + r, j = 16 * J + c;
        float v = acc[s][r];
        if (i < f && j < f) {
          if (i == j) v += reg;
          // both triangles from one accumulator entry (tiles summed from the split path are not bit-symmetric
          // inside a diagonal tile; als.h:39-143 mirrors one temp as well)
          if (I != J || i <= j) {
            if (packed) {  // row i keeps columns i .. f - 1 (cumf_get_hermitian_packed)
              tt[(size_t)i * f - (size_t)(i * (i - 1) / 2) + (j - i)] = (T)v;
            } else {
              tt[(size_t)i * f + j] = (T)v;  // T = _Float16: round to nearest even, as __float2half_rn (als.h:373-499)
              if (i != j) tt[(size_t)j * f + i] = (T)v;
            }
          }
        } else if (i < f && j == f && rhs != nullptr) {
          rhs[i] = v;
        }
      }
    }
  });
}

// Partial tiles <-> global scratch, in accumulator layout ([slot][tile][reg][lane]:
// every store/load is one coalesced 256-byte wave access).
template <int NB, int W>
__device__ __forceinline__ void tiles_to_partial(const f32x4 (&acc)[Geo<NB>::TPW], float* __restrict__ part,
                                                 int lane) {
  constexpr int NT = Geo<NB>::NT, TPW = Geo<NB>::TPW;
  static_for<TPW>([&](auto sc) {
    constexpr int s = decltype(sc)::value;
    constexpr int t = Geo<NB>::tile(W, s);
    if constexpr (t < NT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) part[((size_t)t * 4 + r) * 64 + lane] = acc[s][r];
    }
  });
}
// NEG: the sum of the partial tiles NEGATED (what the blocked workgroup LU eliminates: lu_solve_blocked_wg)
template <int NB, int W, bool NEG = false>
__device__ __forceinline__ void partial_accumulate(f32x4 (&acc)[Geo<NB>::TPW], const float* __restrict__ part,
                                                   int lane) {
  constexpr int NT = Geo<NB>::NT, TPW = Geo<NB>::TPW;
  static_for<TPW>([&](auto sc) {
    constexpr int s = decltype(sc)::value;
    constexpr int t = Geo<NB>::tile(W, s);
    if constexpr (t < NT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = part[((size_t)t * 4 + r) * 64 + lane];
        acc[s][r] = NEG ? acc[s][r] - v : acc[s][r] + v;
      }
    }
  });
}

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

// ----------------------------------------------------------------------------------
// Row epilogue.  dump_row<W> is per-wave (tile layout); solve_row is common to all waves.
// ----------------------------------------------------------------------------------
template <int NB, int MODE, int W>
__device__ __forceinline__ void dump_row(const f32x4 (&acc)[Geo<NB>::TPW], float* smem, const KernelArgs& a, int row,
                                         int rowlen, int lane) {
  const int f = a.f;
  if constexpr (MODE == kModeMaterialize) {
    // als.cu:547: float temp = (end - start) * lambda;
    const float reg = (float)rowlen * a.lambda;
    const size_t off = (size_t)(row - a.row_begin) * (a.tt_packed ? (size_t)f * (f + 1) / 2 : (size_t)f * f);
    float* rhs = a.rhs ? a.rhs + (size_t)(row - a.row_begin) * f : nullptr;
    if (a.tt_half)
      tiles_to_global<NB, W>(acc, reinterpret_cast<_Float16*>(a.tt) + off, rhs, f, reg, lane);
    else
      tiles_to_global<NB, W>(acc, a.tt + off, rhs, f, reg, lane, a.tt_packed != 0);
  } else {
    // G / the tile store aliases the stage buffers (all MFMA reads are done)
    if constexpr (MODE == kModeLU)
      tiles_to_tiled<NB, W>(acc, smem, (float)rowlen * a.lambda, lane);
    else
      tiles_to_lds<NB, W>(acc, smem, solve_ldg(f, MODE), f, (float)rowlen * a.lambda, lane);
  }
}

// LU (default build): the whole solve runs on the accumulators inside the wave roles.
template <int NB, int MODE, int W, bool NEG = false>
__device__ __forceinline__ void finish_row(f32x4 (&acc)[Geo<NB>::TPW], float* smem, const KernelArgs& a, int row,
                                           int rowlen, int tid) {
  if constexpr (MODE == kModeLU && lu_on_accumulators(NB)) {
    lu_solve_wg<NB, W, 4, NEG>(acc, smem, a.f, (float)rowlen * a.lambda, a.update + (size_t)row * a.f, tid, a.sse_bins, rowlen);
  } else {
    dump_row<NB, MODE, W>(acc, smem, a, row, rowlen, tid & 63);
  }
}

template <int NB, int MODE>
__device__ __forceinline__ void solve_row(float* smem, const KernelArgs& a, int row, int tid) {
  if constexpr (MODE == kModeLU && lu_on_accumulators(NB)) return;  // done in finish_row
  if constexpr (MODE != kModeMaterialize) {
    const int f = a.f, ldg = solve_ldg(f, MODE);
    float* G = smem;
    __syncthreads();  // all tiles are in G
    float* x = a.update + (size_t)row * f;
    if constexpr (MODE == kModeCG)
      cg_solve_lds<NB>(G, ldg, f, smem + solve_g_floats(f, MODE), x, a.cg_iters, tid);
    else
      lu_solve_reg<NB>(TileLoad<NB>{smem, f}, smem, f, smem + lu_packed_floats(NB), x, tid);
  }
}

// ----------------------------------------------------------------------------------
// Kernel 1: one workgroup per plan item (a whole row, or one chunk of a heavy row).
// The four waves run wave-specialised copies of the same loop (each owns a fixed set of
// tiles); every copy executes the same sequence of barriers.
// ----------------------------------------------------------------------------------
template <int NB, typename VT, int MODE, int W>
__device__ __forceinline__ void item_body(float* smem, const KernelArgs& a, int row, long long begin, int len,
                                          int slot, int rowlen, int tid) {
  constexpr int LD = Geo<NB>::LD, TPW = Geo<NB>::TPW;
  constexpr int kStageFloats = kStage * LD;
  constexpr int NG = kStage / 4;  // MFMA groups of 4 ratings per full stage
  using St = Stager<NB, VT>;
  const int lane = tid & 63;
  const int f = a.f;
  const unsigned f4 = (unsigned)f * 4u;
  f32x4 acc[TPW];
#pragma unroll
  for (int s = 0; s < TPW; ++s) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nstages = (len + kStage - 1) / kStage;
  auto nvalid_of = [&](int s) { return (len - s * kStage) < kStage ? (len - s * kStage) : kStage; };
  auto begin_of = [&](int s) { return begin + (long long)s * kStage; };
  St st;
  st.init(f, tid);
  // landing slot for masked-off stage stores: inside the read-ahead pad behind the two stage
  // buffers (read by nobody's MFMAs; in fused modes it is overwritten by G only after the
  // last barrier of the loop)
  float* dummy = smem + 2 * kStageFloats + 4 * LD + (tid & 15) * 4;
  // Prologue: padding zeroed, stage 0 into LDS buffer 0, stage 1 gathers in flight, column
  // indices of stage 2.
  if (nstages > 0) {
    const int nv = nvalid_of(0);
    st.template load_cols_into<false>(st.cols, a.colidx, begin, nv);
    st.zero_padding(smem, f, tid);
    st.template gather<false>(a.val, a.gather, f4, begin, nv, tid);
    if (nstages > 1) st.template load_cols_into<false>(st.cols_nx, a.colidx, begin_of(1), nvalid_of(1));
    st.store_masked(smem, dummy, f, nv, (nv + 3) & ~3, tid);
    if (nstages > 1) {
      st.rotate_cols();
      st.template gather<false>(a.val, a.gather, f4, begin_of(1), nvalid_of(1), tid);
      if (nstages > 2) st.template load_cols_into<false>(st.cols, a.colidx, begin_of(2), nvalid_of(2));
    }
  }
  __syncthreads();

  // Steady state.  Every stage but the last is full (32 ratings = NG groups).  While the
  // MFMAs of group g drain through the matrix pipe the wave issues one slice of the staging
  // work: the LDS store of pass p of stage s+1 (gathered during stage s-1, so it has landed)
  // immediately followed by the gather of pass p of stage s+2 into the same registers; the
  // column indices of stage s+3 go out with the first slice.
  const float* rowbase = smem + (lane >> 4) * LD + (lane & 15);
  auto load_blk = [&](float (&blk)[NB], const float* p) {
#pragma unroll
    for (int b = 0; b < NB; ++b) blk[b] = p[16 * b];
  };
  // TARGET_FULL: stage s+1 (the one being stored) holds 32 ratings -> select-free stores.
  auto stage_body = [&](auto fullc, int s) {
    constexpr bool TARGET_FULL = decltype(fullc)::value;
    const float* cur = rowbase + (s & 1) * kStageFloats;
    float* nxt = smem + ((s + 1) & 1) * kStageFloats;
    const int nv1 = nvalid_of(s + 1), nw1 = (nv1 + 3) & ~3;
    // stages s+2 / s+3 may not exist near the end of the item: the loads are then issued
    // anyway on the last existing stage (in-bounds, never stored) to keep the loop branch-free
    const int s2 = (s + 2 < nstages) ? s + 2 : nstages - 1;
    const int s3 = (s + 3 < nstages) ? s + 3 : nstages - 1;
    const int nv2 = nvalid_of(s2), nv3 = nvalid_of(s3);
    const long long b2 = begin_of(s2), b3 = begin_of(s3);
    float blk_a[NB], blk_b[NB];
    load_blk(blk_a, cur);
    static_for<NG>([&](auto gc) {
      constexpr int g = decltype(gc)::value;
      float (&bc)[NB] = (g & 1) ? blk_b : blk_a;
      float (&bn)[NB] = (g & 1) ? blk_a : blk_b;
      if constexpr (g + 1 < NG) load_blk(bn, cur + (g + 1) * 4 * LD);
      __builtin_amdgcn_sched_barrier(0);
      mma_group<NB, W>(bc, acc);
      __builtin_amdgcn_sched_barrier(0);
      static_for<St::PASSES>([&](auto pc) {
        constexpr int p = decltype(pc)::value;
        if constexpr (p * NG / St::PASSES == g) {
          if constexpr (TARGET_FULL)
            st.template store_pass_full<p>(nxt, dummy);
          else
            st.template store_pass_masked<p>(nxt, dummy, nv1, nw1);
          st.template gather_pass<p>(a.gather, f4);
        }
      });
      if constexpr (g == NG - 1) {  // all passes stored: the rating register is free again
        if constexpr (TARGET_FULL)
          st.store_val_full(nxt, f, tid);
        else
          st.store_val_masked(nxt, dummy, f, nv1, nw1, tid);
        st.template gather_val<false>(a.val, b2, nv2, tid);
      }
      if constexpr (g == 0) st.template load_cols_into<false>(st.cols_nx, a.colidx, b3, nv3);  // used a stage later
      __builtin_amdgcn_sched_barrier(0);
    });
    st.rotate_cols();
    __syncthreads();
  };
  for (int s = 0; s + 2 < nstages; ++s) stage_body(std::true_type{}, s);
  if (nstages > 1) stage_body(std::false_type{}, nstages - 2);  // its target is the (ragged) last stage
  if (nstages > 0) {
    const int sl = nstages - 1;
    mma_stage<NB, W>(smem + (sl & 1) * kStageFloats, acc, (nvalid_of(sl) + 3) >> 2, lane);
    __syncthreads();  // every wave is done with the stage buffers (G aliases them)
  }
  if (slot >= 0)
    tiles_to_partial<NB, W>(acc, a.part + (size_t)slot * Geo<NB>::NT * 256, lane);
  else
    finish_row<NB, MODE, W>(acc, smem, a, row, rowlen, tid);
}

template <int NB, typename VT, int MODE>
__global__ __launch_bounds__(kThreads) void als_item_kernel(const KernelArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const int item = blockIdx.x;
  const int row = a.item_row[item];
  const long long begin = a.item_begin[item];
  const int len = a.item_len[item];
  const int slot = a.item_slot[item];
  const int rowlen = a.item_rowlen[item];
  // Role of this wave.  The LU on the accumulators loads the roles unevenly (the last role's tiles
  // stay live to the end), so the roles are rotated with the workgroup index: workgroups that
  // share a CU differ in item / 256 (dispatch is round-robin over 8 XCDs x 32 CUs) and their
  // heavy roles then sit on different SIMDs.
  const int role =
      (MODE == kModeLU && lu_on_accumulators(NB)) ? (((tid >> 6) + (item >> 8) + (item >> 10)) & 3) : (tid >> 6);
  switch (role) {
    case 0: item_body<NB, VT, MODE, 0>(smem, a, row, begin, len, slot, rowlen, tid); break;
    case 1: item_body<NB, VT, MODE, 1>(smem, a, row, begin, len, slot, rowlen, tid); break;
    case 2: item_body<NB, VT, MODE, 2>(smem, a, row, begin, len, slot, rowlen, tid); break;
    default: item_body<NB, VT, MODE, 3>(smem, a, row, begin, len, slot, rowlen, tid); break;
  }
  if (slot < 0) solve_row<NB, MODE>(smem, a, row, tid);
}

// ----------------------------------------------------------------------------------
// Kernel 2: one workgroup per chunked row: sum the partial tiles in slot order (a
// fixed, deterministic order) and finish the row.
// ----------------------------------------------------------------------------------
template <int NB, int MODE, int W>
__device__ __forceinline__ void reduce_body(float* smem, const KernelArgs& a, int row, int slot0, int nslots,
                                            int rowlen, int lane) {
  constexpr int TPW = Geo<NB>::TPW;
  constexpr bool NEG = MODE == kModeLU && lu_on_accumulators(NB) && lu_wg_blocked(NB);  // the blocked LU eliminates -A
  f32x4 acc[TPW];
#pragma unroll
  for (int s = 0; s < TPW; ++s) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int sl = 0; sl < nslots; ++sl)
    partial_accumulate<NB, W, NEG>(acc, a.part + (size_t)(slot0 + sl) * Geo<NB>::NT * 256, lane);
  finish_row<NB, MODE, W, NEG>(acc, smem, a, row, rowlen, lane + 64 * W);
}

// Round 6: the LU of the largest systems (NB = 12, 13: f = 176 .. 207; 164-168 registers = three workgroups per CU) is latency- and
// barrier-bound at full clock (61 % of its wave-cycles parked, profiles/r05/f200_lu/pmc_sq.txt): a fourth workgroup per CU is
// worth more than the registers it spills at 128 (118 at NB = 13, 28 at NB = 12; NB <= 11 fit anyway) -- Netflix f = 200 LU
// Theta side 74.5 -> 71.4 ms (profiles/r06/ab_r13w4.txt).
template <int NB, int MODE>
#ifndef CUMF_REDUCE_LU_WGS
#define CUMF_REDUCE_LU_WGS 4
#endif
__global__ __launch_bounds__(kThreads, (NB >= 11 && MODE == kModeLU) ? CUMF_REDUCE_LU_WGS : 1) void als_reduce_kernel(const KernelArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int mr = blockIdx.x;
  const int row = a.mrow_row[mr];
  const int slot0 = a.dense_slots ? mr : a.mrow_slot0[mr];
  const int nslots = a.dense_slots ? 1 : a.mrow_nslots[mr];
  const int rowlen = a.mrow_rowlen[mr];
  // Role of this wave, rotated with the workgroup index as in als_item_kernel: the LU loads the roles unevenly (role 0 runs
  // the back substitution alone, the owner of a diagonal tile eliminates the pivot blocks), and the waves of a workgroup go
  // to fixed SIMDs -- without the rotation one SIMD of every CU carries all the heavy roles.
  const int role = (MODE == kModeLU && lu_on_accumulators(NB)) ? (((tid >> 6) + (mr >> 8) + (mr >> 10)) & 3) : (tid >> 6);
  switch (role) {
    case 0: reduce_body<NB, MODE, 0>(smem, a, row, slot0, nslots, rowlen, lane); break;
    case 1: reduce_body<NB, MODE, 1>(smem, a, row, slot0, nslots, rowlen, lane); break;
    case 2: reduce_body<NB, MODE, 2>(smem, a, row, slot0, nslots, rowlen, lane); break;
    default: reduce_body<NB, MODE, 3>(smem, a, row, slot0, nslots, rowlen, lane); break;
  }
  solve_row<NB, MODE>(smem, a, row, tid);
}

// ----------------------------------------------------------------------------------
// Standalone batched solvers on materialised systems (the reference's data flow).
// ----------------------------------------------------------------------------------
template <int NB, int MODE>
__global__ __launch_bounds__(kThreads) void solve_lds_kernel(const float* __restrict__ A, const float* __restrict__ b,
                                                             float* __restrict__ x, int f, int cg_iters, int a_half) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const size_t sys = blockIdx.x;
  const float* As = A + sys * (size_t)f * f;  // (fp32 layout; the fp16 layout is indexed below)
  if constexpr (NB != 0 && MODE == kModeLU) {
    lu_solve_reg<NB>(GlobalLoad<NB>{As, b + sys * f, f}, smem, f, smem + lu_packed_floats(NB), x + sys * f,
                               tid);
    return;
  }
  const int ldg = solve_ldg(f, MODE);
  float* G = smem;
  if (a_half) {  // updateXWithCGKernel3 (cg.cu:235-429): A stored as half, arithmetic in fp32
    const _Float16* Ah = reinterpret_cast<const _Float16*>(A) + sys * (size_t)f * f;
    for (int e = tid; e < f * f; e += kThreads) {
      const int i = e / f, j = e - i * f;
      G[i * ldg + j] = (float)Ah[e];
    }
  } else {
    for (int e = tid; e < f * f; e += kThreads) {
      const int i = e / f, j = e - i * f;
      G[i * ldg + j] = As[e];
    }
  }
  if (tid < f) G[tid * ldg + f] = b[sys * f + tid];
  __syncthreads();
  if constexpr (NB == 0)
    lu_solve_lds(G, ldg, f, x + sys * f, tid);
  else if constexpr (MODE == kModeCG)
    cg_solve_lds<NB>(G, ldg, f, smem + solve_g_floats(f, MODE), x + sys * f, cg_iters, tid);
}

// ----------------------------------------------------------------------------------
// Launchers: the per-NB entry points (als_internal.h), called through with_nb by als_launch.cpp
// ----------------------------------------------------------------------------------
template <int NB, typename VT, int MODE>
static hipError_t launch_nb(const KernelArgs& a, long n_items, long n_mrows, hipStream_t stream) {
  const size_t stage_floats = (2 * (size_t)kStage + 8) * Geo<NB>::LD;  // + read-ahead pad of mma_stage
  size_t floats = stage_floats;
  if (MODE != kModeMaterialize) {
    const size_t solve = MODE == kModeLU ? lu_fused_lds_floats<NB>(a.f) : solve_lds_floats(a.f, MODE);
    floats = floats > solve ? floats : solve;
  }
  const size_t lds = floats * sizeof(float);
  if (n_items > 0) {
    hipError_t e = launch_item_kernel(als_item_kernel<NB, VT, MODE>, dim3((unsigned)n_items), dim3(kThreads), lds, stream, a);
    if (e != hipSuccess) return e;
  }
  if (n_mrows > 0) {
    const size_t lds2 = (MODE == kModeMaterialize) ? 0 : lds;
    return launch_kernel(als_reduce_kernel<NB, MODE>, dim3((unsigned)n_mrows), dim3(kThreads), lds2, stream, a);
  }
  return hipSuccess;
}

// the workgroup kernels: the items (als_item_kernel), then the chunked rows (als_reduce_kernel)
template <int NB>
hipError_t slice_half_iteration(const KernelArgs& a, int mode, long n_items, long n_mrows, hipStream_t stream) {
  const bool v4 = (a.f % 4 == 0);
  if (mode == kModeMaterialize)
    return v4 ? launch_nb<NB, f32x4, kModeMaterialize>(a, n_items, n_mrows, stream)
              : launch_nb<NB, f32x2, kModeMaterialize>(a, n_items, n_mrows, stream);
  if constexpr (NB <= kMaxFusedNB) {
    if (mode == kModeCG && a.f <= kVecLd)  // cg_solve_lds holds two vector elements per lane: f <= 128
      return v4 ? launch_nb<NB, f32x4, kModeCG>(a, n_items, n_mrows, stream)
                : launch_nb<NB, f32x2, kModeCG>(a, n_items, n_mrows, stream);
  }
  // the register LU keeps only the packed upper triangle in LDS: fused up to f = 200
  if (mode == kModeLU)
    return v4 ? launch_nb<NB, f32x4, kModeLU>(a, n_items, n_mrows, stream)
              : launch_nb<NB, f32x2, kModeLU>(a, n_items, n_mrows, stream);
  return hipErrorInvalidValue;
}

template <int NB, int MODE>
static hipError_t launch_solve_nb(const float* A, const float* b, float* x, long batch, int f, int cg_iters,
                                  hipStream_t stream, int a_half = 0) {
  const size_t floats = NB == 0 ? solve_lds_floats(f, kModeLUExact)
                                : (MODE == kModeLU ? lu_lds_floats(NB, f) : solve_lds_floats(f, MODE));
  const size_t lds = floats * sizeof(float);
  if (lds > 160 * 1024) return hipErrorInvalidValue;
  return launch_kernel(solve_lds_kernel<NB, MODE>, dim3((unsigned)batch), dim3(kThreads), lds, stream, A, b, x, f,
                       cg_iters, a_half);
}

// batched solve of materialised systems: LDS-resident CG (f <= 128) or register-resident LU (f <= 200); NB = 0: the
// oracle-order LU (kModeLUExact)
template <int NB>
hipError_t slice_solve(const float* A, const float* b, float* x, long batch, int f, int mode, int cg_iters,
                       hipStream_t stream) {
  if (mode == kModeCG || mode == kModeCGHalf) {
    if constexpr (NB != 0 && NB <= kMaxFusedNB)
      return launch_solve_nb<NB, kModeCG>(A, b, x, batch, f, cg_iters, stream, mode == kModeCGHalf);
    return hipErrorInvalidValue;
  }
  return launch_solve_nb<NB, kModeLU>(A, b, x, batch, f, cg_iters, stream);
}

// solver of the chunked rows on its own (the items came from the wave kernels): Route::chunked
template <int NB>
hipError_t slice_reduce_only(const KernelArgs& a, int mode, const Route& r, long n_mrows, hipStream_t stream) {
  if (n_mrows <= 0) return hipSuccess;
  if constexpr (NB >= 2) {
    if (r.chunked == kSolveWaveCG) return wave_solve_launch<NB>(a, mode, n_mrows, stream);
  }
  const dim3 grid((unsigned)n_mrows), block(kThreads);
  if (mode == kModeMaterialize) return launch_kernel(als_reduce_kernel<NB, kModeMaterialize>, grid, block, 0, stream, a);
  if (mode == kModeCG) {
    if constexpr (NB <= kMaxFusedNB) {
      if (a.f > kVecLd) return hipErrorInvalidValue;
      const size_t lds = solve_lds_floats(a.f, kModeCG) * sizeof(float);
      return launch_kernel(als_reduce_kernel<NB, kModeCG>, grid, block, lds, stream, a);
    } else {
      return hipErrorInvalidValue;
    }
  }
  const size_t lds = lu_fused_lds_floats<NB>(a.f) * sizeof(float);
  return launch_kernel(als_reduce_kernel<NB, kModeLU>, grid, block, lds, stream, a);
}

// Large systems (f >= 112): the Gram of every row is dumped as accumulator tiles (two waves per item,
// als_wave_multi_kernel) and a solver kernel (single-wave LU up to NB = 10, the 4-wave lu_solve_mfma
// above that, wave-level CG on the tiles) picks them up -- the reference's own data flow ("Gram batch
// in device memory, separate solver", als.cu:782-831), with tiles instead of full f x f matrices and
// in batches of the pooled tile buffer (als_plan.cpp: up to 48 GiB, usually ONE batch).
template <int NB>
hipError_t slice_batched(const KernelArgs& a0, int mode, const Route& r, const PlanLists& L, hipStream_t stream) {
  if constexpr (NB < 2) {
    return hipErrorInvalidValue;
  } else {
  hipError_t e = hipSuccess;
  // 1. chunked rows: their items write the plan's slots, the reduce kernel sums and solves
  if (L.n_citems > 0) {
    KernelArgs a = a0;
    a.item_row = L.c_row;
    a.item_begin = L.c_begin;
    a.item_len = L.c_len;
    a.item_slot = L.c_slot;
    a.item_rowlen = L.c_rowlen;
    e = wave_item_launch<NB>(a, kModeLU, r, false, L.n_citems, stream);  // every item has a slot: nothing is solved in place
    if (e != hipSuccess) return e;
    e = slice_reduce_only<NB>(a0, mode, r, L.n_mrows, stream);
    if (e != hipSuccess) return e;
  }
  // 2. whole rows: solved by the two waves that formed the Gram, in one launch, or through the tile buffer
  if (r.whole == kSolveInKernel) {
    if (L.n_witems <= 0) return hipSuccess;
    KernelArgs a = a0;
    a.item_row = L.w_row;
    a.item_begin = L.w_begin;
    a.item_len = L.w_len;
    a.item_rowlen = L.w_rowlen;
    a.item_slot = nullptr;  // no slots: nothing is dumped
    a.dense_slots = 0;
    return wave_item_launch<NB>(a, mode, r, false, L.n_witems, stream);
  }
  // large LU / materialise (cumf_get_hermitian): in batches of part2_rows dense slots
  for (long w0 = 0; w0 < L.n_witems; w0 += L.part2_rows) {
    const long cnt = L.n_witems - w0 < L.part2_rows ? L.n_witems - w0 : L.part2_rows;
    KernelArgs a = a0;
    a.item_row = L.w_row + w0;
    a.item_begin = L.w_begin + w0;
    a.item_len = L.w_len + w0;
    a.item_rowlen = L.w_rowlen + w0;
    a.item_slot = nullptr;
    a.dense_slots = 1;
    a.part = L.part2;
    a.mrow_row = L.w_row + w0;
    a.mrow_rowlen = L.w_rowlen + w0;
    e = wave_item_launch<NB>(a, kModeLU, r, false, cnt, stream);
    if (e != hipSuccess) return e;
    e = slice_reduce_only<NB>(a, mode, r, cnt, stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
  }
}

// The entry points of this translation unit's NB (Makefile: one object per CUMF_NB_SLICE).  Slice 0 is only the
// oracle-order LU (solve_lds_kernel<0, kModeLU>, CUMF_ALS_LU_EXACT); the NB-independent kernels are in als_common.hip.
#if CUMF_NB_SLICE == 0
template hipError_t slice_solve<0>(const float*, const float*, float*, long, int, int, int, hipStream_t);
#else
template hipError_t slice_half_iteration<CUMF_NB_SLICE>(const KernelArgs&, int, long, long, hipStream_t);
template hipError_t slice_solve<CUMF_NB_SLICE>(const float*, const float*, float*, long, int, int, int, hipStream_t);
template hipError_t slice_reduce_only<CUMF_NB_SLICE>(const KernelArgs&, int, const Route&, long, hipStream_t);
template hipError_t slice_batched<CUMF_NB_SLICE>(const KernelArgs&, int, const Route&, const PlanLists&, hipStream_t);
#endif

}  // namespace cumf
