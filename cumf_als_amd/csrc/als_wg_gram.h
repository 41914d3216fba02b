// als_wg_gram.h -- the Gram pass of one workgroup (als_item_kernel, als_kernels.hip): kStage gathered factor rows at a
// time go global -> registers -> LDS (Stager) while the four wave roles run the SYRK of the stage before on the fp32
// matrix cores (mma_group, mma_stage); item_body is the loop around the two.
#ifndef CUMF_ALS_WG_GRAM_H_
#define CUMF_ALS_WG_GRAM_H_

#include <hip/hip_runtime.h>

#include <type_traits>

#include "als_device.h"
#include "als_internal.h"
#include "als_wg_tiles.h"

namespace cumf {

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

  __device__ __forceinline__ void load_cols_into(int (&dst)[PASSES], const int* __restrict__ colidx, long long begin,
                                                 int nvalid) {
    const int* base = colidx + begin;  // wave-uniform
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int r = rsub + p * RPP;
      dst[p] = base[(unsigned)(r < nvalid ? r : nvalid - 1)];
    }
  }

  // Gather of one stage: pass p loads VW consecutive features of factor row cols[p]; the
  // rating of row (tid & 31) rides along.  Nothing here consumes a loaded value.
  template <int P>
  __device__ __forceinline__ void gather_pass(const float* __restrict__ gat, unsigned f4) {
    const unsigned off = (unsigned)cols[P] * f4 + goff;  // bytes, < 4 GiB
    v[P] = *reinterpret_cast<const VT*>(reinterpret_cast<const char*>(gat) + off);
  }
  __device__ __forceinline__ void gather_val(const float* __restrict__ val, long long begin, int nvalid, int tid) {
    const int r = tid & (kStage - 1);
    if (val == nullptr) {  // no ratings given (alsUpdateFeature100Host: the right-hand side comes precomputed): zeros
      rvv = 0.f;
      return;
    }
    const float* vbase = val + begin;  // wave-uniform
    rvv = vbase[(unsigned)(r < nvalid ? r : nvalid - 1)];
  }
  __device__ __forceinline__ void gather(const float* __restrict__ val, const float* __restrict__ gat, unsigned f4,
                                         long long begin, int nvalid, int tid) {
    static_for<PASSES>([&](auto pc) { gather_pass<decltype(pc)::value>(gat, f4); });
    gather_val(val, begin, nvalid, tid);
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
// SYRK of one stage on the matrix cores.  Wave role W owns the tiles Geo<NB>::tile(W, s).
//   D[i][j] += sum_k A[i][k] B[k][j],  A[i][k] = theta_k[16I+i], B[k][j] = theta_k[16J+j]
// v_mfma_f32_16x16x4_f32 operand layout: lane l supplies A[l&15][l>>4] and
// B[l>>4][l&15]; both are stage[4g + (l>>4)][16*blk + (l&15)], so a feature
// block's register serves as the A operand of its tile row and the B operand of its
// tile column.  Accumulation is the exact k-ordered fmaf chain (rating order).
// ----------------------------------------------------------------------------------
template <int NB, int W>
__device__ __forceinline__ void mma_group(const float (&blk)[NB], f32x4 (&acc)[Geo<NB>::TPW]) {
  for_each_tile<NB, W>([&](auto sc, auto tc) {
    constexpr int s = decltype(sc)::value, t = decltype(tc)::value;
    constexpr int I = tile_I<NB>(t), J = tile_J<NB>(t);
    acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(blk[I], blk[J], acc[s], 0, 0, 0);
  });
}

// One MFMA operand per feature block: element (lane >> 4, lane & 15) of the group of four gathered rows at p.
template <int NB>
__device__ __forceinline__ void load_blk(float (&blk)[NB], const float* p) {
#pragma unroll
  for (int b = 0; b < NB; ++b) blk[b] = p[16 * b];
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

// The row epilogue of the kernel file (als_kernels.hip): solves or dumps the row whose accumulators item_body completed.
template <int NB, int MODE, int W, bool NEG = false>
__device__ __forceinline__ void finish_row(f32x4 (&acc)[Geo<NB>::TPW], float* smem, const KernelArgs& a, int row,
                                           int rowlen, int tid);

// ----------------------------------------------------------------------------------
// One plan item (a whole row, or one chunk of a heavy row) in one workgroup.
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
    st.load_cols_into(st.cols, a.colidx, begin, nv);
    st.zero_padding(smem, f, tid);
    st.gather(a.val, a.gather, f4, begin, nv, tid);
    if (nstages > 1) st.load_cols_into(st.cols_nx, a.colidx, begin_of(1), nvalid_of(1));
    st.store_masked(smem, dummy, f, nv, (nv + 3) & ~3, tid);
    if (nstages > 1) {
      st.rotate_cols();
      st.gather(a.val, a.gather, f4, begin_of(1), nvalid_of(1), tid);
      if (nstages > 2) st.load_cols_into(st.cols, a.colidx, begin_of(2), nvalid_of(2));
    }
  }
  __syncthreads();

  // Steady state.  Every stage but the last is full (32 ratings = NG groups).  While the
  // MFMAs of group g drain through the matrix pipe the wave issues one slice of the staging
  // work: the LDS store of pass p of stage s+1 (gathered during stage s-1, so it has landed)
  // immediately followed by the gather of pass p of stage s+2 into the same registers; the
  // column indices of stage s+3 go out with the first slice.
  const float* rowbase = smem + (lane >> 4) * LD + (lane & 15);
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
        st.gather_val(a.val, b2, nv2, tid);
      }
      if constexpr (g == 0) st.load_cols_into(st.cols_nx, a.colidx, b3, nv3);  // used a stage later
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

}  // namespace cumf

#endif  // CUMF_ALS_WG_GRAM_H_
