// als_wave_pre.h -- the Gram stage of the wave kernels (als_wave.hip) on a PRE-SPLIT gather table (kArithPre, kArithPrePk):
// the stage image in LDS, its 16-byte LDS-DMA gather and transposing reads (PreGeo / PreStage / PreGather), the stage steps
// of the one-wave kernel, and the same construction shared by the two waves of als_wave_multi_kernel (PreGeo2 / PreGather2).
// Product map, schedules and prefetch step: als_wave_gram.h.
#pragma once
#include "als_wave_gram.h"

namespace cumf {

// ----------------------------------------------------------------------------------
// kArithPre / kArithPrePk: the stage on a pre-split gather table (round 6; tools/probes/tr16_dma_probe.hip pins the two
// instructions it is built on).
//
// Table row (presplit_bf16x3_kernel), FB = f / 16 full feature blocks, SP = (f % 16) / 4 in {0, 1} strip pieces:
//   [h: 16 FB bf16][m: 16 FB bf16][l: 16 FB bf16] [strip, if SP: h, m, l of features 16 FB .. 16 FB + 3 (8 B each) + 8 B of zeros]
// LDS image of a 32-rating stage:
//   main    chunk (E, p), E = 0..7, p = plane: the plane of FOUR ratings rho = 4 E + q, q = 0..3, at RP bytes each, written
//           by ONE global_load_lds_dwordx4 (lane l = LP q + piece: 16 bytes -> chunk + 16 l; the lanes behind the 2 FB pieces
//           of a rating are masked off); 24 chunks instead of 56 dword gathers.  RP = 192 (64 for FB <= 2) and a 32-byte
//           skew per E pair put the eight 32-byte row pieces a transposing read touches per half wave into eight bank groups.
//   strip   [rho][h 8 B | m 8 B | l 8 B | pad 8 B] of the 32 ratings: one more 16-byte LDS-DMA (lane l: rating l / 2, half l % 2)
//   rating  the rating value rides in slot f (als.cu:750-757 fused into the Gram) and is no table entry: lane rho splits the
//           value of rating rho of the stage (loaded a stage ahead) and stores it once the stage's chunks have landed --
//           kArithPrePk: [r_h r_m r_l 0] as ONE 8-byte store into the strip's pad; kArithPre: [r_h 0 0 0 | r_m 0 0 0 | r_l 0 0 0]
//   zeros   24 bytes: what the lanes behind slot f read
// Operands: ds_read_b64_tr_b16 hands lane 4 a + b of a 16-lane group, as element j, halfword b of the 8-byte piece that lane
// 4 j + a addresses.  Lane (g, 4 j + a) addresses features 16 B + 4 a .. + 3 of rating rho = 8 g + 4 u + j: lane (g, c) receives
// feature 16 B + c of the ratings 8 g + 4 u + 0 .. 3 -- K slots 4 u .. 4 u + 3 of the MFMA, exactly the slots the in-kernel
// split gives them (P.h[B][2 u], [2 u + 1]).
//   kArithPre    every block like that, the last one from strip / rating pieces per plane: same operands in the same slots,
//                same MFMA sequence -- the accumulators are BIT-IDENTICAL to kArithSplit3's
//                (tests/test_gpu_parity.py::test_presplit_is_bit_identical); the verification form (cumf_set_presplit(2)).
//   kArithPrePk  the production form: the last feature block (f = 100: four features + the rating, 11 of 16 columns zero) is
//                read as ONE packed operand pk whose columns are [h of the strip features | m | l | r_h r_m r_l 0]: tile
//                (I, NB - 1) takes three products h_I pk + m_I pk + l_I pk (all nine plane products at once) instead of six,
//                tile (NB - 1, NB - 1) one (pk pk^T) instead of four -- 133 MFMAs per stage instead of 154 at f = 100 -- and
//                once per item the column groups are folded back (wave_fold_strip).  Error class of kArithSplit3 (the three
//                dropped products ml, lm, ll are now included), not its bits in the last block column.
// ----------------------------------------------------------------------------------
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4* lds_tr_ptr;
typedef char __attribute__((address_space(3)))* lds_byte_ptr;
template <int NB>
struct PreGeo {
  static constexpr int FB = NB - 1;
  static constexpr int RP = FB <= 2 ? 64 : 192;       // bytes of one rating inside a chunk (>= 32 FB)
  static constexpr int LP = RP / 16;                  // DMA lanes per rating, 2 FB of them fetch
  static constexpr int CS = 4 * RP;                   // one chunk: a plane of four ratings
  static constexpr int kMain = 24 * CS + 3 * 32;      // + the skews: chunk (E, p) at (3 E + p) CS + 32 (E >> 1)
  static constexpr int kStrip = kMain;                // 32 ratings x 32 B
  static constexpr int kZero = kStrip + 1024;         // 24 B (32 reserved)
  static constexpr int kRating = kZero + 32;          // kArithPre only: 32 ratings x 24 B
  __host__ __device__ static constexpr int bytes(bool packed) { return packed ? kRating : kRating + 768; }
  static_assert(32 * FB <= RP && 4 * LP <= 64, "a rating's plane fits its slot, four ratings fit the wave");
  __host__ __device__ static constexpr int chunk(int E, int p) { return (3 * E + p) * CS + 32 * (E >> 1); }
};

template <int NB>
struct PreStage {
  int idx[8];   // column indices of the ratings 4 E + q of a stage whose main chunks are still to be issued (lanes of DMA group q)
  int sidx;     // ... of rating lane / 2 (strip)
  float rv;     // rating value of rating lane & 31 of the stage whose chunks are in flight
};
template <int NB, bool PK>
struct PreGather {
  using G = PreGeo<NB>;
  const char* lane_base;   // table + 16 piece
  const char* zero_base;   // zero row + 16 piece
  const char* strip_base;  // table + 96 FB + 16 (lane & 1)
  const char* strip_zero;
  const int* ib;           // colidx + begin (the zero row for an item without ratings)
  const float* vb;         // val + begin (the zero row without ratings / values)
  lds_tr_ptr tr_main;      // lane part of the addresses of the transposing reads of blocks 0 .. FB - 1
  lds_tr_ptr tr_last[2];   // ... of the last block, per quad u
  unsigned pitch;
  int len, q, lane;
#if CUMF_ABLATE_STAGE
  int dbg;
#endif
  bool dma_active, sp;

  __device__ __forceinline__ void init(const KernelArgs& a, int f, long long begin, int len_, int lane_, float* smem) {
    lane = lane_;
    len = len_;
    pitch = a.pre_pitch;
#if CUMF_ABLATE
    if (a.dbg & 8) pitch = 0u;  // profiling build: 8 = every gather hits row 0
#endif
#if CUMF_ABLATE_STAGE
    dbg = a.dbg;
#endif
    sp = ((f & 15) >> 2) != 0;
    q = lane / G::LP;
    const int piece = lane % G::LP;
    dma_active = q < 4 && piece < 2 * G::FB;
    q = q < 4 ? q : 3;
    lane_base = reinterpret_cast<const char*>(a.gather) + 16 * piece;
    zero_base = reinterpret_cast<const char*>(g_wave_zeros) + 16 * piece;
    strip_base = reinterpret_cast<const char*>(a.gather) + 96 * G::FB + 16 * (lane & 1);
    strip_zero = reinterpret_cast<const char*>(g_wave_zeros) + 16 * (lane & 1);
    ib = len_ > 0 ? a.colidx + begin : reinterpret_cast<const int*>(g_wave_zeros);
    vb = (len_ > 0 && a.val != nullptr) ? a.val + begin : g_wave_zeros;
    const int g = lane >> 4, j = (lane >> 2) & 3, aa = lane & 3;
    lds_byte_ptr base = (lds_byte_ptr)smem;
    tr_main = (lds_tr_ptr)(base + 6 * g * G::CS + 32 * g + G::RP * j + 8 * aa);
    const int spn = sp ? 1 : 0;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int rho = 8 * g + 4 * u + j;
      int off;
      if constexpr (PK)  // columns [h feats | m feats | l feats | rating]: the strip's pieces in order, the rating piece in its pad
        off = (sp || aa == 0) ? G::kStrip + 32 * rho + (sp ? 8 * aa : 24) : G::kZero;
      else
        off = aa < spn ? G::kStrip + 32 * rho + 8 * aa : (aa == spn ? G::kRating + 24 * rho : G::kZero);
      tr_last[u] = (lds_tr_ptr)(base + off);
    }
    // the zero pieces (and the rating pieces' zero halfwords), once (LDS operations of one wave execute in order)
    constexpr int kClear = (G::bytes(PK) - G::kZero) / 16;
    if (lane < kClear) reinterpret_cast<f32x4*>(reinterpret_cast<char*>(smem) + G::kZero)[lane] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // column indices of stage s (FULL: every rating of the stage exists)
  template <bool FULL>
  __device__ __forceinline__ void load_idx(PreStage<NB>& st, int s) const {
    const int top = len > 0 ? len - 1 : 0;
    if constexpr (FULL) {
      const int* p = ib + kWaveStage * s + q;
#pragma unroll
      for (int E = 0; E < 8; ++E) st.idx[E] = p[4 * E];
      st.sidx = ib[kWaveStage * s + (lane >> 1)];
    } else {
#pragma unroll
      for (int E = 0; E < 8; ++E) {
        const int pos = kWaveStage * s + 4 * E + q;
        st.idx[E] = ib[pos < top ? pos : top];
      }
      const int ps = kWaveStage * s + (lane >> 1);
      st.sidx = ib[ps < top ? ps : top];
    }
  }
  // rating value of stage s; ratings past the end of the item: zero rows AND a zero rating (sum r^2 of the fused SSE)
  template <bool FULL>
  __device__ __forceinline__ void load_rv(PreStage<NB>& st, int s) const {
    const int pv = kWaveStage * s + (lane & 31);
    if constexpr (FULL) {
      st.rv = vb[pv];
    } else {
      const int top = len > 0 ? len - 1 : 0;
      const float v = vb[pv < top ? pv : top];
      st.rv = pv < len ? v : 0.f;
    }
  }

  // the rating values of the stage that has just landed (st.rv) as three bf16 terms into its rating pieces
  __device__ __forceinline__ void put_rating(const PreStage<NB>& st, float* smem) const {
    unsigned H, M, L;
    split3_pair(st.rv, 0.f, H, M, L);
    if (lane < 32) {
      if constexpr (PK) {
        u32x2 w = {(H & 0xffffu) | (M << 16), L & 0xffffu};
        *reinterpret_cast<u32x2*>(reinterpret_cast<char*>(smem) + G::kStrip + 32 * lane + 24) = w;
      } else {
        unsigned short* rp = reinterpret_cast<unsigned short*>(reinterpret_cast<char*>(smem) + G::kRating + 24 * lane);
        rp[0] = (unsigned short)H;
        rp[4] = (unsigned short)M;
        rp[8] = (unsigned short)L;
      }
    }
  }

  template <bool FULL>
  __device__ __forceinline__ void dma_issue(const PreStage<NB>& st, float* smem, int s) const {
#if defined(__HIP_DEVICE_COMPILE__)  // (the host pass of hipcc rejects the 16-byte form of the builtin: it checks it against the host target)
    using gptr = const __attribute__((address_space(1))) void*;
    using lptr = __attribute__((address_space(3))) void*;
    lds_byte_ptr lds = (lds_byte_ptr)smem;
    if (dma_active) {
      static_for<8>([&](auto ec) {
        constexpr int E = decltype(ec)::value;
        const char* row = lane_base + (unsigned long long)(unsigned)st.idx[E] * pitch;  // v_mad_u64_u32
        if constexpr (!FULL) row = (kWaveStage * s + 4 * E + q < len) ? row : zero_base;
        static_for<3>([&](auto pc) {
          constexpr int p = decltype(pc)::value;
          // the instruction offset (the plane's byte offset in the row) moves BOTH addresses: taken back out of the LDS pointer
          __builtin_amdgcn_global_load_lds((gptr)row, (lptr)(lds + G::chunk(E, p) - 32 * G::FB * p), 16, 32 * G::FB * p, 0);
        });
      });
    }
    if (sp) {  // wave-uniform
      const char* row = strip_base + (unsigned long long)(unsigned)st.sidx * pitch;
      if constexpr (!FULL) row = (kWaveStage * s + (lane >> 1) < len) ? row : strip_zero;
      __builtin_amdgcn_global_load_lds((gptr)row, (lptr)(lds + G::kStrip), 16, 0, 0);
    }
#endif
  }

  // the landed stage -> MFMA operands
  static __device__ __forceinline__ u32x2 tr_read(lds_tr_ptr p, int byte_off) {
    return __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)((lds_byte_ptr)p + byte_off)));
  }
  // the planes of the full blocks B0 .. B1 - 1
  template <int B0, int B1, class PL>
  __device__ __forceinline__ void read_blocks(PL& P) const {
    static_for<B1 - B0>([&](auto bc) {
      constexpr int B = B0 + decltype(bc)::value;
      static_for<2>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const u32x2 vh = tr_read(tr_main, (3 * u + 0) * G::CS + 32 * B);
        const u32x2 vm = tr_read(tr_main, (3 * u + 1) * G::CS + 32 * B);
        const u32x2 vl = tr_read(tr_main, (3 * u + 2) * G::CS + 32 * B);
        P.h[B][2 * u] = vh[0], P.h[B][2 * u + 1] = vh[1];
        P.m[B][2 * u] = vm[0], P.m[B][2 * u + 1] = vm[1];
        P.l[B][2 * u] = vl[0], P.l[B][2 * u + 1] = vl[1];
      });
    });
  }
  template <class PL>
  __device__ __forceinline__ void read_pk(PL& P) const {  // the packed last block (kArithPrePk)
    const u32x2 v0 = tr_read(tr_last[0], 0), v1 = tr_read(tr_last[1], 0);
    P.pk = u32x4{v0[0], v0[1], v1[0], v1[1]};
  }
  template <class PL>
  __device__ __forceinline__ void read(PL& P) const {
    if constexpr (PK) read_pk(P);
    static_for<G::FB>([&](auto bc) {
      constexpr int B = decltype(bc)::value;
      static_for<2>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const u32x2 vh = tr_read(tr_main, (3 * u + 0) * G::CS + 32 * B);
        const u32x2 vm = tr_read(tr_main, (3 * u + 1) * G::CS + 32 * B);
        const u32x2 vl = tr_read(tr_main, (3 * u + 2) * G::CS + 32 * B);
        P.h[B][2 * u] = vh[0], P.h[B][2 * u + 1] = vh[1];
        P.m[B][2 * u] = vm[0], P.m[B][2 * u + 1] = vm[1];
        P.l[B][2 * u] = vl[0], P.l[B][2 * u + 1] = vl[1];
      });
    });
    // the last block (no generic lambda here: the form not taken must be discarded, not just skipped)
    if constexpr (!PK) {
      constexpr int B = G::FB;
      const u32x2 h0 = tr_read(tr_last[0], 0), m0 = tr_read(tr_last[0], 8), l0 = tr_read(tr_last[0], 16);
      const u32x2 h1 = tr_read(tr_last[1], 0), m1 = tr_read(tr_last[1], 8), l1 = tr_read(tr_last[1], 16);
      P.h[B] = u32x4{h0[0], h0[1], h1[0], h1[1]};
      P.m[B] = u32x4{m0[0], m0[1], m1[0], m1[1]};
      P.l[B] = u32x4{l0[0], l0[1], l1[0], l1[1]};
    }
  }
};

// One stage: wait for the chunks -> rating pieces -> 6 NB transposing reads -> chunks of the next stage, indices of the one
// after, rating values of the next -> MFMAs.  At entry R holds the indices of stage s_next and the rating values of this one.
template <int NB, int KIND, bool PK, class PL>
__device__ __forceinline__ void stage_step_pre(const PreGather<NB, PK>& wg, PL& P, PreStage<NB>& R, float* smem,
                                               f32x4 (&acc)[NB * (NB + 1) / 2], int s_next, int s_load) {
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the chunks of this stage have landed, R is complete
  wg.put_rating(R, smem);
  wg.read(P);
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the operands are in registers, the image is free
  if constexpr (KIND == kStepFull) {
    wg.template dma_issue<true>(R, smem, s_next);
    wg.template load_idx<true>(R, s_load);
    wg.template load_rv<true>(R, s_next);
  } else if constexpr (KIND == kStepPartial) {
    const int nfull = wg.len / kWaveStage, nst = (wg.len + kWaveStage - 1) / kWaveStage;
    if (s_next < nfull) {
      wg.template dma_issue<true>(R, smem, s_next);
      wg.template load_rv<true>(R, s_next);
    } else {
      wg.template dma_issue<false>(R, smem, s_next);
      wg.template load_rv<false>(R, s_next);
    }
    if (s_load < nfull)
      wg.template load_idx<true>(R, s_load);
    else if (s_load < nst)
      wg.template load_idx<false>(R, s_load);
  }
  u32x4 h2[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
  static_for<GramSched<NB>::N>([&](auto nc) { gram_mfma_sched<NB, GramSched, decltype(nc)::value>(P, acc, h2); });
}

// kArithPrePk: the same step with the MFMAs in two groups around the prefetch (GramSchedPk) -- the first group needs
// only the operands of the first blocks and runs under the transposing reads of the others.
template <int NB, int KIND>
__device__ __forceinline__ void stage_step_pk(const PreGather<NB, true>& wg, Planes<NB, kArithPrePk>& P, PreStage<NB>& R,
                                              float* smem, f32x4 (&acc)[NB * (NB + 1) / 2], int s_next, int s_load) {
  constexpr GramSchedPk<NB> S = GramSchedPk<NB>::make();
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the chunks of this stage have landed, R is complete
  wg.put_rating(R, smem);
  constexpr int FB = NB - 1, HB = GramSchedPk<NB>::HB, kLate = 6 * (FB - HB);  // transposing reads of the second group's blocks
  u32x4 h2[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
#if CUMF_ABLATE_STAGE  // one-off timing builds only (tools/wave_variants.sh EXTRA="-DCUMF_ABLATE=1 -DCUMF_ABLATE_STAGE=1"): a
  // switch inside the stage changes its scheduling regions, so the profiling build proper has none here
  if (wg.dbg & 32) {  // 32 = no transposing reads (the operands keep the first stage's values)
    static_for<S.n1>([&](auto nc) { gram_mfma_sched<NB, GramSchedPk, decltype(nc)::value>(P, acc, h2); });
  } else
#endif
  {
    wg.read_pk(P);
    wg.template read_blocks<0, HB>(P);
    __builtin_amdgcn_sched_barrier(0);
    // One region: the reads of the other blocks go out ONE BEHIND EACH of the first MFMAs (at most 16 LDS operations are in
    // flight per wave -- a burst of reads in front of the MFMAs would hold the wave until all but 16 have returned)
    wg.template read_blocks<HB, FB>(P);
    static_for<S.n1>([&](auto nc) { gram_mfma_sched<NB, GramSchedPk, decltype(nc)::value>(P, acc, h2); });
    static_for<(kLate < S.n1 ? kLate : S.n1)>([&](auto) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // one MFMA
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // one LDS read
    });
  }
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): every operand is in registers, the image is free
  if constexpr (KIND == kStepFull) {
#if CUMF_ABLATE_STAGE
    if (!(wg.dbg & 16))  // 16 = no LDS-DMA in the steady state
#endif
    wg.template dma_issue<true>(R, smem, s_next);
    wg.template load_idx<true>(R, s_load);
    wg.template load_rv<true>(R, s_next);
  } else if constexpr (KIND == kStepPartial) {
    const int nfull = wg.len / kWaveStage, nst = (wg.len + kWaveStage - 1) / kWaveStage;
    if (s_next < nfull) {
      wg.template dma_issue<true>(R, smem, s_next);
      wg.template load_rv<true>(R, s_next);
    } else {
      wg.template dma_issue<false>(R, smem, s_next);
      wg.template load_rv<false>(R, s_next);
    }
    if (s_load < nfull)
      wg.template load_idx<true>(R, s_load);
    else if (s_load < nst)
      wg.template load_idx<false>(R, s_load);
  }
  static_for<GramSchedPk<NB>::N - S.n1>([&](auto nc) { gram_mfma_sched<NB, GramSchedPk, S.n1 + decltype(nc)::value>(P, acc, h2); });
}

// ----------------------------------------------------------------------------------
// kArithPre for the two-wave kernel (round 6): the stage image of the pre-split table is SHARED by the two waves of the item.
// Same construction as PreGather, sized for FB = 7 .. 12 full blocks: a rating's plane (32 FB bytes) sits in a slot of RP =
// 320 (FB <= 9) or 448 bytes, chunk (E, p) = plane p of the four ratings 4 E + q as before; wave W fetches the ratings
// q = 2 W, 2 W + 1 of every chunk (one global_load_lds_dwordx4 per (E, p) and wave: 24 per stage and wave instead of 52 dword
// gathers), the strip of the ratings 16 W .. 16 W + 15 (64 bytes per rating: h | m | l of up to eight features + 16 zero
// bytes) and their rating values.  ONE stage buffer, two barriers per stage: chunks landed + rating pieces written ->
// barrier -> both waves read ALL blocks (6 NB transposing reads, no split: the 468 VALU instructions per stage and wave of
// the in-kernel form are gone) -> barrier -> the chunks of the next stage -> this wave's MFMAs, which cover the gather.
// The last block is read per plane (strip pieces | the rating piece [r_p 0 0 0] | zeros): the same operands in the same K
// slots as the in-kernel split, the same MFMA order per tile -- bit-identical accumulators.
// ----------------------------------------------------------------------------------
template <int NB>
struct PreGeo2 {
  static constexpr int FB = NB - 1;
  static constexpr int RP = FB <= 9 ? 320 : 448;      // = 64 or 192 (mod 256): four ratings -> four 64-byte bank groups
  static constexpr int LP = RP / 16;
  static constexpr int CS = 4 * RP;
  static constexpr int kMain = 24 * CS + 3 * 32;
  static constexpr int kStrip = kMain;                // 32 ratings x 64 B
  static constexpr int kZero = kStrip + 2048;         // 64 B
  static constexpr int kRating = kZero + 64;          // 32 ratings x 3 planes x 16 B
  static constexpr int kBytes = kRating + 1536;
  static_assert(32 * FB <= RP && 2 * LP <= 64, "a rating's plane fits its slot, two ratings fit the wave");
  __host__ __device__ static constexpr int chunk(int E, int p) { return (3 * E + p) * CS + 32 * (E >> 1); }
};

template <int NB, int W>
struct PreGather2 {
  using G = PreGeo2<NB>;
  const char* lane_base;
  const char* zero_base;
  const char* strip_base;
  const char* strip_zero;
  const int* ib;
  const float* vb;
  lds_tr_ptr tr_main, tr_last[2];
  unsigned pitch;
  int len, q, lane;
  bool dma_active, sp;

  __device__ __forceinline__ void init(const KernelArgs& a, int f, long long begin, int len_, int lane_, float* smem) {
    lane = lane_;
    len = len_;
    pitch = a.pre_pitch;
    const int spn = (f & 15) >> 2;  // strip pieces per plane: 0, 1 or 2
    sp = spn != 0;
    const int piece = lane % G::LP;
    q = 2 * W + (lane / G::LP < 2 ? lane / G::LP : 1);
    dma_active = lane < 2 * G::LP && piece < 2 * G::FB;
    lane_base = reinterpret_cast<const char*>(a.gather) + 16 * piece;
    zero_base = reinterpret_cast<const char*>(g_wave_zeros) + 16 * piece;
    strip_base = reinterpret_cast<const char*>(a.gather) + 96 * G::FB + 16 * (lane & 3);
    strip_zero = reinterpret_cast<const char*>(g_wave_zeros) + 16 * (lane & 3);
    ib = len_ > 0 ? a.colidx + begin : reinterpret_cast<const int*>(g_wave_zeros);
    vb = (len_ > 0 && a.val != nullptr) ? a.val + begin : g_wave_zeros;
    const int g = lane >> 4, j = (lane >> 2) & 3, aa = lane & 3;
    lds_byte_ptr base = (lds_byte_ptr)smem;
    tr_main = (lds_tr_ptr)(base + 6 * g * G::CS + 32 * g + G::RP * j + 8 * aa);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int rho = 8 * g + 4 * u + j;
      const int off = aa < spn ? G::kStrip + 64 * rho + 8 * aa : (aa == spn ? G::kRating + 48 * rho : G::kZero);
      tr_last[u] = (lds_tr_ptr)(base + off);
    }
    // the zero halfwords of this wave's rating pieces (16 ratings x 48 B) and, wave 0, the zero pieces -- once; each wave only
    // clears what it alone writes afterwards, the barrier of the first stage publishes it
    if (lane < 48) reinterpret_cast<f32x4*>(reinterpret_cast<char*>(smem) + G::kRating + 768 * W)[lane] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (W == 0 && lane < 4) reinterpret_cast<f32x4*>(reinterpret_cast<char*>(smem) + G::kZero)[lane] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  __device__ __forceinline__ void load_idx(PreStage<NB>& st, int s) const {
    const int top = len > 0 ? len - 1 : 0;
#pragma unroll
    for (int E = 0; E < 8; ++E) {
      const int pos = kWaveStage * s + 4 * E + q;
      st.idx[E] = ib[pos < top ? pos : top];
    }
    const int ps = kWaveStage * s + 16 * W + (lane >> 2);
    st.sidx = ib[ps < top ? ps : top];
  }
  __device__ __forceinline__ void load_rv(PreStage<NB>& st, int s) const {
    const int top = len > 0 ? len - 1 : 0;
    const int pv = kWaveStage * s + 16 * W + (lane & 15);
    const float v = vb[pv < top ? pv : top];
    st.rv = pv < len ? v : 0.f;
  }
  __device__ __forceinline__ void put_rating(const PreStage<NB>& st, float* smem) const {
    unsigned H, M, L;
    split3_pair(st.rv, 0.f, H, M, L);
    if (lane < 16) {
      unsigned short* rp = reinterpret_cast<unsigned short*>(reinterpret_cast<char*>(smem) + G::kRating + 48 * (16 * W + lane));
      rp[0] = (unsigned short)H;
      rp[8] = (unsigned short)M;
      rp[16] = (unsigned short)L;
    }
  }
  __device__ __forceinline__ void dma_issue(const PreStage<NB>& st, float* smem, int s) const {
#if defined(__HIP_DEVICE_COMPILE__)
    using gptr = const __attribute__((address_space(1))) void*;
    using lptr = __attribute__((address_space(3))) void*;
    lds_byte_ptr lds = (lds_byte_ptr)smem;
    if (dma_active) {
      static_for<8>([&](auto ec) {
        constexpr int E = decltype(ec)::value;
        const char* row = lane_base + (unsigned long long)(unsigned)st.idx[E] * pitch;
        row = (kWaveStage * s + 4 * E + q < len) ? row : zero_base;
        static_for<3>([&](auto pc) {
          constexpr int p = decltype(pc)::value;
          __builtin_amdgcn_global_load_lds((gptr)row, (lptr)(lds + G::chunk(E, p) + 2 * W * G::RP - 32 * G::FB * p), 16, 32 * G::FB * p, 0);
        });
      });
    }
    if (sp) {  // wave-uniform: the strip of the ratings 16 W .. 16 W + 15
      const char* row = strip_base + (unsigned long long)(unsigned)st.sidx * pitch;
      row = (kWaveStage * s + 16 * W + (lane >> 2) < len) ? row : strip_zero;
      __builtin_amdgcn_global_load_lds((gptr)row, (lptr)(lds + G::kStrip + 1024 * W), 16, 0, 0);
    }
#endif
  }
  static __device__ __forceinline__ u32x2 tr_read(lds_tr_ptr p, int byte_off) {
    return __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)((lds_byte_ptr)p + byte_off)));
  }
  template <int B0, int B1>
  __device__ __forceinline__ void read_blocks(Planes<NB>& P) const {
    static_for<B1 - B0>([&](auto bc) {
      constexpr int B = B0 + decltype(bc)::value;
      static_for<2>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const u32x2 vh = tr_read(tr_main, (3 * u + 0) * G::CS + 32 * B);
        const u32x2 vm = tr_read(tr_main, (3 * u + 1) * G::CS + 32 * B);
        const u32x2 vl = tr_read(tr_main, (3 * u + 2) * G::CS + 32 * B);
        P.h[B][2 * u] = vh[0], P.h[B][2 * u + 1] = vh[1];
        P.m[B][2 * u] = vm[0], P.m[B][2 * u + 1] = vm[1];
        P.l[B][2 * u] = vl[0], P.l[B][2 * u + 1] = vl[1];
      });
    });
  }
  __device__ __forceinline__ void read_last(Planes<NB>& P) const {
    constexpr int B = G::FB;
    const u32x2 h0 = tr_read(tr_last[0], 0), m0 = tr_read(tr_last[0], 16), l0 = tr_read(tr_last[0], 32);
    const u32x2 h1 = tr_read(tr_last[1], 0), m1 = tr_read(tr_last[1], 16), l1 = tr_read(tr_last[1], 32);
    P.h[B] = u32x4{h0[0], h0[1], h1[0], h1[1]};
    P.m[B] = u32x4{m0[0], m0[1], m1[0], m1[1]};
    P.l[B] = u32x4{l0[0], l0[1], l1[0], l1[1]};
  }
};

// LDS floats of one stage of the one-wave kernel (and of one of the two stage buffers of the two-wave kernel's dword form)
template <int NB, int ARITH = kArithSplit3>
__host__ __device__ constexpr int wave_stage_lds_floats() {
  if constexpr (ARITH == kArithPre || ARITH == kArithPrePk)
    return PreGeo<NB>::bytes(ARITH == kArithPrePk) / 4;  // the pre-split image of a stage
  else
    return 64 * 8 * NB;             // 8 NB chunks of 64 floats
}

}  // namespace cumf
