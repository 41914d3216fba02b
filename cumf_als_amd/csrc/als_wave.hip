// als_wave.hip -- wave-level ALS half-iteration kernels for gfx950 (16 <= f <= 207).
//
// Same job as als_item_kernel (als_kernels.hip) -- RHS + Gram + solve of one plan item,
// replacing cusparseScsrmm2 + cublasSgeam (als.cu:750-757), get_hermitian100 /
// get_hermitianT10 (als.cu:443-569 / 575-659), the batched LU (als.cu:58-189) and the CG of
// cg.cu:36-231 -- with a different mapping onto the chip:
//
//   * als_wave_kernel (NB = 2 .. 7, f <= 111): ONE wave owns one item and all NB (NB + 1) / 2
//     upper-triangular 16 x 16 accumulator tiles of its system.  No workgroup barrier anywhere: every
//     lane gathers straight into the MFMA operand layout, a full stage ahead of its use and through LDS.
//     als_wave_multi_kernel (NB = 8 .. 13): two waves per item share the chunks and split the tiles.
//   * The Gram stage -- fp32 on the bf16 matrix pipe: als_wave_gram.h (the in-kernel split of the fp32 gather table) and
//     als_wave_pre.h (the pre-split table).
//   * The tile epilogues and the CG on the accumulators: als_wave_solve.h.  The LU on the accumulators: als_wave_lu.h.
//
// This file: the kernels, the body of the two-wave kernel, the launchers and the explicit instantiations of this
// translation unit's NB and part.
//
// The accumulator layout (C/D of every 16 x 16 MFMA: lane (g, c), register r = element
// (4 g + r, c)) and the partial-tile scratch layout are those of als_kernels.hip, so chunked
// rows go through the same als_reduce_kernel.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <type_traits>

#ifndef CUMF_WAVE_NB
#error "compile with -DCUMF_WAVE_NB=<feature blocks>"
#endif

#include "als_device.h"
#include "als_lu_wg.h"
#include "als_lu_blocked.h"
#include "als_internal.h"
#include "als_wave_gram.h"
#include "als_wave_pre.h"
#include "als_wave_solve.h"

namespace cumf {

// feature-block counts whose kernels also exist on the pre-split table (kArithPre): f = 96 .. 111 and f = 64 .. 79 -- the
// headline f = 100 and BASELINE configs[4]'s f = 64 (presplit_nb_ok in als_internal.h is the host's copy of this list)
#define CUMF_WAVE_PRE (CUMF_WAVE_NB == 7 || CUMF_WAVE_NB == 5)
// feature-block counts with kArithSplitPk instances (the in-kernel split with the rating-only last block packed, f % 16 == 0)
#define CUMF_WAVE_SPLITPK (CUMF_WAVE_NB <= 7)

template <int NB, int NW>
__global__ __launch_bounds__(64 * NW, 2) void als_wave_cg_kernel(const KernelArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63;
  const int mr = blockIdx.x;
  const int row = a.mrow_row[mr];
  const int slot0 = a.dense_slots ? mr : a.mrow_slot0[mr];
  const int nslots = a.dense_slots ? 1 : a.mrow_nslots[mr];
  const int rowlen = a.mrow_rowlen[mr];
  if constexpr (NW == 1) {
    cg_wave_body<NB, 1, 0>(smem, a, row, slot0, nslots, rowlen, lane);
  } else if constexpr (NW == 2) {
    if ((threadIdx.x >> 6) == 0)
      cg_wave_body<NB, NW, 0>(smem, a, row, slot0, nslots, rowlen, lane);
    else
      cg_wave_body<NB, NW, 1>(smem, a, row, slot0, nslots, rowlen, lane);
  } else {
    static_assert(NW == 4, "1, 2 or 4 waves per system");
    switch (threadIdx.x >> 6) {
      case 0: cg_wave_body<NB, NW, 0>(smem, a, row, slot0, nslots, rowlen, lane); break;
      case 1: cg_wave_body<NB, NW, 1>(smem, a, row, slot0, nslots, rowlen, lane); break;
      case 2: cg_wave_body<NB, NW, 2>(smem, a, row, slot0, nslots, rowlen, lane); break;
      default: cg_wave_body<NB, NW, 3>(smem, a, row, slot0, nslots, rowlen, lane); break;
    }
  }
}

// ----------------------------------------------------------------------------------
// Kernel: one 64-thread workgroup (= one wave) per plan item.  FC != 0: f known at compile time.
// ----------------------------------------------------------------------------------
#define CUMF_WAVE_MIN_WAVES 2
// kArithFast epilogue of the Gram pass: the accumulators carry 4096^2 x the Gram; a rating beyond the
// f16 range (|r| >= 15.99; the table is checked by presplit_f16x2_kernel) shows as a non-finite
// right-hand side (column f lives in the tiles of the last block column) and is reported through
// a.fast_flag (cumf_gram_fast_status).  NW, W: tile t belongs to wave t % NW, slot t / NW.
template <int NB, int NW, int W>
__device__ __forceinline__ void fast_unscale(f32x4 (&acc)[(NB * (NB + 1) / 2 + NW - 1) / NW], int* flag) {
  constexpr int NT = NB * (NB + 1) / 2, TPW = (NT + NW - 1) / NW;
  float probe = 0.f;
  static_for<TPW>([&](auto sc) {
    constexpr int sl = decltype(sc)::value, t = W + NW * sl;
    if constexpr (t < NT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[sl][r] *= kFastUnscale;
      if constexpr (tile_J<NB>(t) == NB - 1) probe += (acc[sl][0] + acc[sl][1]) + (acc[sl][2] + acc[sl][3]);
    }
  });
  if (!(__builtin_fabsf(probe) <= 3.0e38f)) atomicOr(flag, 2);
}

// WHOLE: every item of the launch is a whole row (the plan has no chunked rows: the Netflix Theta side, the
// hugewiki X side).  The kernel then has no "dump the partial tiles" exit between the Gram pass and the solver,
// and THAT exit is what made the register allocator relocate the accumulator tiles at the hand-over and park
// five of them in scratch (41 spilled registers, 2.9 GB of scratch writes per Netflix Theta launch; 0 without it).
// (the CG instances of the small systems sit at the edge of three waves per SIMD -- 166 registers at NB = 5 -- and the packed form
// went over it: 174 registers, Theta side 4.6 -> 4.95 ms at f = 64; held at three)
// PANEL: the LU eliminates sixteen pivots per step (kLuPanel16) -- als_wave_kernel where lu16_default(NB) -- or four
// (kLuPanel4; als_wave_kernel_p4: the instances CUMF_ALS_LU16=0 routes to).
template <int NB, int MODE, int FC, int ARITH, bool WHOLE, LuPanel PANEL>
__device__ __forceinline__ void wave_kernel_body(const KernelArgs& a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NT = NB * (NB + 1) / 2;
  const int lane = threadIdx.x;
  const int item = blockIdx.x;
  const int row = a.item_row[item];
  const long long begin = a.item_begin[item];
  const int len = a.item_len[item];
  const int slot = WHOLE ? -1 : (a.dense_slots ? item : a.item_slot[item]);
  const int rowlen = a.item_rowlen[item];
  const int f = FC ? FC : a.f;
  // (A static s_setprio for the wave in the odd hardware slot, meant to break a lockstep of the two waves
  // of a SIMD, measured neutral to slightly negative -- X side 6.70 vs 6.57 ms without it -- and is gone.)

  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // at least one stage, also for a row without ratings (it gathers the zero row: see WaveGather::init)
  const int nst = len > 0 ? (len + kWaveStage - 1) / kWaveStage : 1;
  const int nfull = len / kWaveStage;
#if CUMF_ABLATE
  // the profiling build only (libALS_ablate.so, -DCUMF_ABLATE=1; results are wrong on purpose): 2 = no Gram pass
  if (!(a.dbg & 2))
#endif
  {
    auto clamp = [&](int s) { return s < nst ? s : nst - 1; };
    if constexpr (ARITH == kArithPre || ARITH == kArithPrePk) {
      constexpr bool PK = ARITH == kArithPrePk;
      PreGather<NB, PK> wg;
      wg.init(a, f, begin, len, lane, smem);
      PreStage<NB> R;
      Planes<NB, PK ? kArithPrePk : kArithSplit3> P;
      // prologue: chunks of stage 0 in flight, its rating values, the indices of stage 1
      wg.template load_idx<false>(R, 0);
      wg.template dma_issue<false>(R, smem, 0);
      wg.template load_rv<false>(R, 0);
      wg.template load_idx<false>(R, clamp(1));
      int s = 0;
      if constexpr (PK) {
        for (; s + 2 < nfull; ++s) stage_step_pk<NB, kStepFull>(wg, P, R, smem, acc, s + 1, s + 2);
        for (; s + 1 < nst; ++s) stage_step_pk<NB, kStepPartial>(wg, P, R, smem, acc, s + 1, s + 2);
        stage_step_pk<NB, kStepLast>(wg, P, R, smem, acc, 0, 0);
        wave_fold_strip<NB>(acc, wg.sp, lane);
      } else {
        for (; s + 2 < nfull; ++s) stage_step_pre<NB, kStepFull, PK>(wg, P, R, smem, acc, s + 1, s + 2);
        for (; s + 1 < nst; ++s) stage_step_pre<NB, kStepPartial, PK>(wg, P, R, smem, acc, s + 1, s + 2);
        stage_step_pre<NB, kStepLast, PK>(wg, P, R, smem, acc, 0, 0);
      }
    } else {
    constexpr bool SPK = ARITH == kArithSplitPk;
    WaveGather<NB, SPK> wg;
    wg.init(a, f, begin, len, lane);
    WaveStage<NB> R;
    Planes<NB, ARITH> P;
    lds_float_ptr lds = (lds_float_ptr)smem;  // staging chunks of this wave (the LU window aliases them later)
    const float* lds_lane = smem + lane;
    // prologue: chunks + ratings of stage 0 in flight, indices of stage 1
    wg.template load_idx<false>(R, 0);
    wg.template dma_issue<false>(R, lds, 0);
    wg.template load_rv<false>(R, 0);
    wg.template load_idx<false>(R, clamp(1));
    const int c = lane & 15;
    // stages s + 1, s + 2 full: select-free steps; then the clamped form; the last stage of the item
    // prefetches nothing (three step bodies, each branch-free)
    int s = 0;
    for (; s + 2 < nfull; ++s) stage_step<NB, kStepFull, ARITH>(wg, P, R, lds, lds_lane, acc, s + 1, s + 2, c);
    for (; s + 1 < nst; ++s) stage_step<NB, kStepPartial, ARITH>(wg, P, R, lds, lds_lane, acc, s + 1, s + 2, c);
    stage_step<NB, kStepLast, ARITH>(wg, P, R, lds, lds_lane, acc, 0, 0, c);
    if constexpr (SPK) wave_fold_strip<NB>(acc, false, lane);
    }
  }
  if constexpr (ARITH == kArithFast) fast_unscale<NB, 1, 0>(acc, a.fast_flag);
  if constexpr (ARITH != kArithFast) {
#if CUMF_ABLATE
    if (!(a.dbg & 2))
#endif
      wave_symmetrise_diag<NB>(acc, smem, lane);
  }

  if constexpr (!WHOLE) {
    if (slot >= 0) {
      wave_tiles_to_partial<NB>(acc, a.part + (size_t)slot * NT * 256, lane);
      return;
    }
  }
  const float reg = (float)rowlen * a.lambda;  // als.cu:547: (end - start) * lambda
#if CUMF_ABLATE
  if (a.dbg & 1) {  // ablation: no solve (keep the accumulators alive)
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) sum += (acc[t][0] + acc[t][1]) + (acc[t][2] + acc[t][3]);
    if (lane < f) a.update[(size_t)row * f + lane] = sum;
    return;
  }
#endif
  if constexpr (MODE == kModeMaterialize) {
    const size_t off = (size_t)(row - a.row_begin) * (a.tt_packed ? (size_t)f * (f + 1) / 2 : (size_t)f * f);
    float* rhs = a.rhs ? a.rhs + (size_t)(row - a.row_begin) * f : nullptr;
    if (a.tt_half)
      wave_tiles_to_global<NB>(acc, reinterpret_cast<_Float16*>(a.tt) + off, rhs, f, reg, lane);
    else
      wave_tiles_to_global<NB>(acc, a.tt + off, rhs, f, reg, lane, a.tt_packed != 0);
  } else if constexpr (MODE == kModeCG) {
    cg_wave_core<NB, 1, 0>(acc, smem, a, f, row, rowlen, lane);  // the reference's default solver (als.cu:28)
  } else {
    const float ssq = lu_wave_blocked<NB, FC, PANEL>(acc, smem, f, reg, a.update + (size_t)row * f, lane, a.dbg);
    constexpr float ff_sign = -1.0f;  // the blocked elimination works on the negated system
    if (a.sse_bins != nullptr) {  // fused train SSE: (f, f) of the eliminated system - reg (1 + |theta|^2)
      const float ff = ff_sign * wave_tile_ff<NB>(acc[NT - 1], f);
      const float tt = wave_sum_uniform(ssq);
      wave_sse_add(a.sse_bins, (double)ff - (double)reg * (1.0 + (double)tt), rowlen, lane);
    }
  }
}
template <int NB, int MODE, int FC, int ARITH = kArithSplit3, bool WHOLE = false>
__global__ __launch_bounds__(64, (NB <= 5 && MODE == kModeCG) ? 3 : CUMF_WAVE_MIN_WAVES) void als_wave_kernel(const KernelArgs a) {
  wave_kernel_body<NB, MODE, FC, ARITH, WHOLE, (MODE == kModeLU && lu16_default(NB)) ? kLuPanel16 : kLuPanel4>(a);
}
template <int NB, int MODE, int FC, int ARITH, bool WHOLE>
__global__ __launch_bounds__(64, CUMF_WAVE_MIN_WAVES) void als_wave_kernel_p4(const KernelArgs a) {
  wave_kernel_body<NB, MODE, FC, ARITH, WHOLE, kLuPanel4>(a);
}

// ----------------------------------------------------------------------------------
// Large systems (NB = 8 .. 13, f = 112 .. 207): NW = 2 waves per item.  The upper-triangular tiles
// are dealt to the two waves (tile t belongs to wave t % 2: 46 / 45 tiles at NB = 13), both waves
// need every feature block of the stage as an operand, so the 8 NB gather chunks are shared: each
// wave issues the LDS-DMA loads of its half of the chunks, two workgroup barriers per stage make the
// hand-over (all chunks landed / all chunks read), and each wave splits all blocks for itself
// (redundant VALU: the alternative is a third pass through LDS).  No solve in this kernel: every
// item dumps its tiles (plan slots for chunk items, dense slots for whole rows) and
// als_reduce_kernel finishes the rows (LU, CG for f <= 128, or the materialised f x f Gram for
// cg_global_kernel) -- the reference's own data flow (als.cu:782-831).
// ----------------------------------------------------------------------------------
template <int NB, int NW, int W, int MODE, int ARITH>
__device__ __forceinline__ void multi_body(float* smem, const KernelArgs& a, long long begin, int len, int slot,
                                           int row, int rowlen, int lane) {
  constexpr int NT = NB * (NB + 1) / 2;
  constexpr int TPW = (NT + NW - 1) / NW;
  const int f = a.f;
  f32x4 acc[TPW];
#pragma unroll
  for (int s = 0; s < TPW; ++s) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nst = len > 0 ? (len + kWaveStage - 1) / kWaveStage : 1;  // a row without ratings: one stage on zeros
  if constexpr (ARITH == kArithPre) {
    PreGather2<NB, W> wg;
    wg.init(a, f, begin, len, lane, smem);
    PreStage<NB> R;
    Planes<NB> P;
    auto clamp = [&](int s) { return s < nst ? s : nst - 1; };
    wg.load_idx(R, 0);
    wg.dma_issue(R, smem, 0);
    wg.load_rv(R, 0);
    wg.load_idx(R, clamp(1));
    for (int s = 0; s < nst; ++s) {
      // this wave's MFMAs in two groups (as the one-wave stage_step_pk): the tiles among the first HB blocks run under the
      // transposing reads of the other blocks; the order of the six products of any one tile is unchanged
      constexpr int HB = NB / 2;
      auto group = [&](auto first) {
        constexpr bool FIRST = decltype(first)::value;
        static_for<6>([&](auto pc) {
          constexpr int PROD = decltype(pc)::value;
          static_for<TPW>([&](auto sc) {
            constexpr int t = W + NW * decltype(sc)::value;
            if constexpr (t < NT) {
              constexpr int I = tile_I<NB>(t), J = tile_J<NB>(t), sl = decltype(sc)::value;
              if constexpr ((J < HB) == FIRST) {
                gram_apply<PROD, I, J>(P, acc[sl]);
              }
            }
          });
        });
      };
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's chunks of stage s, its indices of s + 1, its rating values of s
      wg.put_rating(R, smem);
      __syncthreads();                      // ... and the partner's; the rating pieces of both
      wg.template read_blocks<0, HB>(P);
      __builtin_amdgcn_sched_barrier(0);
      wg.template read_blocks<HB, NB - 1>(P);
      wg.read_last(P);
      group(std::true_type{});
      static_for<6 * (NB - HB)>([&](auto) {  // the late reads one behind each of the first MFMAs (<= 16 LDS operations in flight)
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      });
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_waitcnt(0xC07F);
      __syncthreads();                      // both waves have their operands: the image is free
      if (s + 1 < nst) {                    // uniform
        wg.dma_issue(R, smem, s + 1);
        wg.load_idx(R, clamp(s + 2));
        wg.load_rv(R, s + 1);
      }
      group(std::false_type{});
    }
    __syncthreads();  // (the solvers alias the image: nobody may still be reading the last stage's pieces -- they are not, but the
                      // CG's exchange buffer and the LU's are written right away)
  } else {
    WaveGather<NB> wg;
    wg.init(a, f, begin, len, lane);
    WaveStage<NB> R;
    Planes<NB, ARITH> P;
    using gptr = const __attribute__((address_space(1))) void*;
    using lptr = __attribute__((address_space(3))) void*;
    auto clamp = [&](int s) { return s < nst ? s : nst - 1; };
    // this wave's share of the chunks of stage s (feature blocks b with b % NW == W)
    // two stage buffers: the chunks of stage s + 1 are issued before stage s is converted (a full
    // conversion + MFMA phase of lead time, one workgroup barrier per stage)
    constexpr int kBuf = wave_stage_lds_floats<NB>();
    auto issue_share = [&](int s, int buf) {
      lds_float_ptr lds = (lds_float_ptr)smem + buf * kBuf;
      static_for<8>([&](auto ec) {
        constexpr int E = decltype(ec)::value;
        const char* row = wg.template row_ptr<false, E>(R, s);
        static_for<NB>([&](auto bc) {
          constexpr int B = decltype(bc)::value;
          if constexpr (B % NW == W) {
            constexpr int k = E * NB + B;
            if constexpr (B + 1 < NB)
              __builtin_amdgcn_global_load_lds((gptr)row, (lptr)(lds + 64 * k - 16 * B), 4, 64 * B, 0);
            else
              __builtin_amdgcn_global_load_lds((gptr)(row + wg.last_off), (lptr)(lds + 64 * k), 4, 0, 0);
          }
        });
      });
    };
    wg.template load_idx<false>(R, 0);
    issue_share(0, 0);
    wg.template load_rv<false>(R, 0);
    wg.template load_idx<false>(R, clamp(1));
    for (int s = 0; s < nst; ++s) {
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's chunks of stage s (and the indices of s + 1) are here
      __syncthreads();                      // ... and the partner's; everybody is done reading stage s - 1
      if (s + 1 < nst) issue_share(s + 1, (s + 1) & 1);  // uniform: the last stage prefetches nothing
      const float* lds_lane = smem + (s & 1) * kBuf + lane;
      // chunk -> registers -> planes, block by block (the raw values of one block live at a time)
      static_for<NB>([&](auto bc) {
        constexpr int B = decltype(bc)::value;
        static_for<8>([&](auto ec) {
          constexpr int E = decltype(ec)::value;
          R.raw[B][E] = lds_lane[64 * (E * NB + B)];
        });
        if constexpr (B == NB - 1) static_for<8>([&](auto ec) { wg.template finish_one<decltype(ec)::value, ARITH>(R); });
        static_for<4>([&](auto vc) { split_pair<NB, B, decltype(vc)::value>(R, P); });
      });
      if (s + 1 < nst) {
        wg.template load_rv<false>(R, s + 1);
        wg.template load_idx<false>(R, clamp(s + 2));
      }
      static_for<gram_products<ARITH>()>([&](auto pc) {
        constexpr int PROD = decltype(pc)::value;
        static_for<TPW>([&](auto sc) {
          constexpr int t = W + NW * decltype(sc)::value;
          if constexpr (t < NT) {
            constexpr int I = tile_I<NB>(t), J = tile_J<NB>(t), sl = decltype(sc)::value;
            // (the four-product form of the diagonal tiles -- GramSched -- was measured here too, round 5: 13 of 91 tiles, the
            // doubled plane recomputed per product, one more barrier per item: f = 200 X side 29.73 vs 29.75 ms, Theta side CG
            // 36.0 vs 35.6, f = 128 LU 26.9 vs 26.9 -- no gain with one wave per SIMD, not kept)
            gram_apply<gram_kind<ARITH>(PROD), I, J>(P, acc[sl]);
          }
        });
      });
    }
  }
  if constexpr (ARITH == kArithFast) fast_unscale<NB, NW, W>(acc, a.fast_flag);
  // a whole row (no slot): the two waves solve it where the tiles are -- 93 KB per row at f = 200 that
  // neither go out to HBM nor come back (measured: 45 GB each way per Netflix X half-iteration)
  if (slot < 0) {
#if CUMF_ABLATE
    if (a.dbg & 1) {  // ablation: no solve (keep the accumulators alive)
      float sum = 0.f;
#pragma unroll
      for (int s = 0; s < TPW; ++s) sum += (acc[s][0] + acc[s][1]) + (acc[s][2] + acc[s][3]);
      if (64 * W + lane < f) a.update[(size_t)row * f + 64 * W + lane] = sum;
      return;
    }
#endif
    if constexpr (MODE == kModeCG) {
      cg_wave_core<NB, NW, W>(acc, smem, a, f, row, rowlen, lane);
    } else {
      __syncthreads();  // the partner is done with the stage buffers: the LU's exchange buffers alias them
      lu_solve_wg<NB, W, NW>(acc, smem, f, (float)rowlen * a.lambda, a.update + (size_t)row * f, lane, a.sse_bins, rowlen);
    }
    return;
  }
  float* part = a.part + (size_t)slot * NT * 256;
  static_for<TPW>([&](auto sc) {
    constexpr int t = W + NW * decltype(sc)::value;
    if constexpr (t < NT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) part[((size_t)t * 4 + r) * 64 + lane] = acc[decltype(sc)::value][r];
    }
  });
}

template <int NB, int NW, int MODE, int ARITH = kArithSplit3>
__global__ __launch_bounds__(64 * NW, NB >= 10 ? 1 : 2) void als_wave_multi_kernel(const KernelArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x;
  const long long begin = a.item_begin[item];
  const int len = a.item_len[item];
  const int slot = a.dense_slots ? item : (a.item_slot ? a.item_slot[item] : -1);
  const int row = a.item_row[item];
  const int rowlen = a.item_rowlen[item];
  static_assert(NW == 2, "two waves per item");
  if ((threadIdx.x >> 6) == 0)
    multi_body<NB, NW, 0, MODE, ARITH>(smem, a, begin, len, slot, row, rowlen, lane);
  else
    multi_body<NB, NW, 1, MODE, ARITH>(smem, a, begin, len, slot, row, rowlen, lane);
}

// This file is compiled twice per NB <= 7 (Makefile): part 0 holds everything but the LU form of
// als_wave_kernel, part 1 only that (wave_lu_launch), built with -mllvm -enable-misched=false: the pre-RA
// machine scheduler triples the accumulator spills at the Gram -> LU hand-over of that kernel (125 vs 38
// registers; Netflix f = 100 LU 18.4 -> 18.0 ms on the same box) while every other kernel is faster with it
// (f = 100 CG 16.6 vs 18.4, f = 200 CG 67 vs 82).
#ifndef CUMF_WAVE_PART
#define CUMF_WAVE_PART 0
#endif

#if CUMF_WAVE_PART == 0
template <int NB>
hipError_t wave_solve_launch(const KernelArgs& a, int mode, long n_rows, hipStream_t stream) {
  if (n_rows <= 0) return hipSuccess;
  if (mode != kModeCG) return hipErrorInvalidValue;  // LU / materialise of dumped tiles: als_reduce_kernel (als_kernels.hip)
  // the tiles are VALU operands (VGPRs only): 91 tiles at NB = 13 = four waves x 23 tiles next to the five
  // vectors, at two waves per SIMD
  constexpr int NW = NB >= 10 ? 4 : 1;
  const size_t lds = NW > 1 ? (size_t)NW * NB * 16 * sizeof(float) : 0;
  return launch_kernel(als_wave_cg_kernel<NB, NW>, dim3((unsigned)n_rows), dim3(64 * NW), lds, stream, a);
}
#endif  // CUMF_WAVE_PART == 0


// The one decoder of (Route::arith, Route::fc): go(arith, fc) on the instance this slice has, as std::integral_constants;
// hipErrorInvalidValue for any combination it has not.  The FC = 100 instances (the reference's own specialisation,
// get_hermitian100 for f == 100, als.cu:788-817) exist at NB = 7, the pre-split ones at CUMF_WAVE_PRE (one wave) and on
// two waves (kArithPre only), the packed in-kernel split at CUMF_WAVE_SPLITPK (f % 16 == 0: FC = 0 only).
template <class Go>
static hipError_t with_arith(const Route& r, Go&& go) {
  auto at = [&](auto arith) -> hipError_t {
    if (r.fc == 0) return go(arith, std::integral_constant<int, 0>{});
    if constexpr (CUMF_WAVE_NB == 7 && decltype(arith)::value != kArithSplitPk) {
      if (r.fc == 100) return go(arith, std::integral_constant<int, 100>{});
    }
    return hipErrorInvalidValue;
  };
  switch (r.arith) {
    case kArithSplit3: return at(std::integral_constant<int, kArithSplit3>{});
    case kArithFast: return at(std::integral_constant<int, kArithFast>{});
#if CUMF_WAVE_PRE || CUMF_WAVE_NB > 7
    case kArithPre: return at(std::integral_constant<int, kArithPre>{});
#endif
#if CUMF_WAVE_PRE
    case kArithPrePk: return at(std::integral_constant<int, kArithPrePk>{});
#endif
#if CUMF_WAVE_SPLITPK
    case kArithSplitPk: return at(std::integral_constant<int, kArithSplitPk>{});
#endif
    default: return hipErrorInvalidValue;
  }
}

#if CUMF_WAVE_PART == 1 && CUMF_WAVE_NB <= 7
// ---- part 1: the LU form of the wave-per-item kernel
template <int NB, int FC, int ARITH, bool WHOLE>
static hipError_t launch_wave_lu_w(const KernelArgs& a, bool lu16, long n_items, hipStream_t stream) {
  const size_t stage_lds = wave_stage_lds_floats<NB, ARITH>() * sizeof(float);
  const size_t lu_lds = wave_lu_lds_floats<NB>(a.f) * sizeof(float);
  const size_t lds = lu_lds > stage_lds ? lu_lds : stage_lds;
  auto kernel = als_wave_kernel<NB, kModeLU, FC, ARITH, WHOLE>;
  if constexpr (lu16_default(NB)) {
    if (!lu16) kernel = als_wave_kernel_p4<NB, kModeLU, FC, ARITH, WHOLE>;  // CUMF_ALS_LU16=0: the four-pivot panels
  }
  if (n_items <= 0) {  // every row of the plan went to the dual-form kernel (als_dual.hip): this is still the route's kernel
    note_item_kernel(reinterpret_cast<const void*>(kernel));
    return hipSuccess;
  }
  return launch_item_kernel(kernel, dim3((unsigned)n_items), dim3(64), lds, stream, a);
}
// whole: no item of this launch dumps partial tiles (WHOLE: the instance without the dump exit)
template <int NB>
hipError_t wave_lu_launch(const KernelArgs& a, const Route& r, bool whole, long n_items, hipStream_t stream) {
  return with_arith(r, [&](auto arith, auto fc) {
    constexpr int ARITH = decltype(arith)::value, FC = decltype(fc)::value;
    return whole ? launch_wave_lu_w<NB, FC, ARITH, true>(a, r.lu16, n_items, stream)
                 : launch_wave_lu_w<NB, FC, ARITH, false>(a, r.lu16, n_items, stream);
  });
}
#endif

#if CUMF_WAVE_PART == 0
// ----------------------------------------------------------------------------------
// Launcher (called by launch_half_iteration, als_launch.cpp)
// ----------------------------------------------------------------------------------
template <int NB, int FC, int ARITH>
static hipError_t launch_wave_fc(const KernelArgs& a, int mode, long n_items, hipStream_t stream) {
  const size_t stage_lds = wave_stage_lds_floats<NB, ARITH>() * sizeof(float);
  if (mode != kModeMaterialize)
    return launch_item_kernel(als_wave_kernel<NB, kModeCG, FC, ARITH>, dim3((unsigned)n_items), dim3(64), stage_lds, stream, a);
  if constexpr (ARITH != kArithSplit3) {
    return hipErrorInvalidValue;  // materialise: the 24-bit arithmetic on the fp32 table only
  } else {
    return launch_item_kernel(als_wave_kernel<NB, kModeMaterialize, FC, kArithSplit3>, dim3((unsigned)n_items), dim3(64),
                              stage_lds, stream, a);
  }
}

template <int NB>
hipError_t wave_item_launch(const KernelArgs& a, int mode, const Route& r, bool whole, long n_items, hipStream_t stream) {
  // (the one-wave LU is also called without items, to name its kernel: launch_wave_lu_w)
  if (n_items <= 0 && !(mode == kModeLU && NB <= kMaxWaveNB && r.n_dual > 0)) return hipSuccess;
  if (mode != kModeMaterialize && mode != kModeLU && mode != kModeCG) return hipErrorInvalidValue;
  if constexpr (NB > kMaxWaveNB) {
    // two waves per item; items without a slot (whole rows) are solved in the kernel (CG, or the LU of
    // als_lu_wg.h with two wave roles), items with one dump their tiles
    return with_arith(r, [&](auto arith, auto) -> hipError_t {
      constexpr int ARITH = decltype(arith)::value;
      if (ARITH != kArithSplit3 && mode == kModeMaterialize) return hipErrorInvalidValue;
      // double-buffered stages of dword chunks, or one stage image of the pre-split table shared by the two waves
      size_t lds = ARITH == kArithPre ? PreGeo2<NB>::kBytes : 2 * wave_stage_lds_floats<NB>() * sizeof(float);
      if (lu_wg_lds_floats<NB>(a.f) * sizeof(float) > lds) lds = lu_wg_lds_floats<NB>(a.f) * sizeof(float);
      const auto kernel = mode == kModeCG ? als_wave_multi_kernel<NB, 2, kModeCG, ARITH>
                                          : als_wave_multi_kernel<NB, 2, kModeLU, ARITH>;
      return launch_item_kernel(kernel, dim3((unsigned)n_items), dim3(128), lds, stream, a);
    });
  } else {
    if (mode == kModeLU) return wave_lu_launch<NB>(a, r, whole, n_items, stream);  // part 1 of this file
    return with_arith(r, [&](auto arith, auto fc) {
      return launch_wave_fc<NB, decltype(fc)::value, decltype(arith)::value>(a, mode, n_items, stream);
    });
  }
}

#endif  // CUMF_WAVE_PART == 0

#if CUMF_ABLATE && CUMF_WAVE_PART == 0
// profiling build: read (and clear) the CG iteration histogram of this feature-block count's kernels
template <int NB>
hipError_t wave_cg_hist(unsigned long long* out16) {
  hipError_t e = hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_cg_hist), 16 * sizeof(unsigned long long));
  if (e != hipSuccess) return e;
  const unsigned long long zero[16] = {};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_cg_hist), zero, sizeof(zero));
}
#endif

#if CUMF_WAVE_PART == 0 && CUMF_WAVE_NB == 7
// ----------------------------------------------------------------------------------
// The gather table as bf16 h | m | l planes (kArithPre; one launch per half-iteration on the launch stream: the factors
// change every half-iteration -- 7 MB read + 11 MB written for the Netflix X table).  One thread per value; the split is
// split3_pair's, the instruction sequence of the in-kernel split: the planes are the same bits.
// ----------------------------------------------------------------------------------
// sw: halfwords per plane in the strip (4: the one-wave kernels' [h 4][m 4][l 4][0 4]; 8: the two-wave kernels'
// [h 8][m 8][l 8][0 8]); what the strip's features do not fill is zero.
__global__ __launch_bounds__(256) void presplit_bf16x3_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst,
                                                              long long n, int f, int fb, int sw, unsigned pitch_halfs) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long row = i / f;
  const int k = (int)(i - row * f);
  unsigned H, M, L;
  split3_pair(src[i], 0.f, H, M, L);
  unsigned short* r = dst + row * pitch_halfs;
  if (k < 16 * fb) {
    r[k] = (unsigned short)H;
    r[16 * fb + k] = (unsigned short)M;
    r[32 * fb + k] = (unsigned short)L;
  } else {
    const int e = k - 16 * fb, sf = f - 16 * fb;
    unsigned short* st = r + 48 * fb;
    st[e] = (unsigned short)H;
    st[sw + e] = (unsigned short)M;
    st[2 * sw + e] = (unsigned short)L;
    if (e == 0) {  // the rest of the strip: zeros
      for (int p = 0; p < 3; ++p)
        for (int z = sf; z < sw; ++z) st[p * sw + z] = 0;
      for (int z = 0; z < sw; ++z) st[3 * sw + z] = 0;
    }
  }
}
hipError_t launch_presplit3(const float* src, void* dst, long long rows, int f, hipStream_t stream) {
  const long long n = rows * f;
  if (n <= 0) return hipSuccess;
  if (!presplit_supported(f)) return hipErrorInvalidValue;
  const int fb = f / 16;
  const unsigned pitch = presplit_pitch(f);
  return launch_kernel(presplit_bf16x3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, src,
                       static_cast<unsigned short*>(dst), n, f, fb, nb_for_f(f) > kMaxWaveNB ? 8 : 4, pitch / 2);
}
#endif

// The entry points of this translation unit's NB and part (als_internal.h)
#if CUMF_WAVE_PART == 0
template hipError_t wave_item_launch<CUMF_WAVE_NB>(const KernelArgs&, int, const Route&, bool, long, hipStream_t);
template hipError_t wave_solve_launch<CUMF_WAVE_NB>(const KernelArgs&, int, long, hipStream_t);
#if CUMF_ABLATE
template hipError_t wave_cg_hist<CUMF_WAVE_NB>(unsigned long long*);
#endif
#elif CUMF_WAVE_NB <= 7
template hipError_t wave_lu_launch<CUMF_WAVE_NB>(const KernelArgs&, const Route&, bool, long, hipStream_t);
#endif

}  // namespace cumf
