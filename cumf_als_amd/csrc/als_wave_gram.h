// als_wave_gram.h -- the Gram stage of the wave kernels (als_wave.hip) on the fp32 gather table: the gather of a 32-rating
// stage through LDS-DMA, the exact bf16x3 split, the map from a product kind to MFMA operands, the MFMA schedules, the
// per-item epilogues of the four-product diagonal tiles and of the packed last block, the stage step and its prefetch.
//
//   * The gather.  Every lane gathers straight into the MFMA operand layout -- lane (g, c) = (lane >> 4, lane & 15)
//     fetches feature 16 b + c of the eight ratings 8 g .. 8 g + 7 of a 32-rating stage, one
//     4-byte global_load_lds_dword per (feature block b, rating): a wave instruction touches four
//     64-byte segments of four gathered factor rows and lands as one 256-byte chunk in LDS, a full
//     stage ahead of its use and without holding registers.  64-bit lane addresses: no 4 GiB limit.
//   * fp32 on the bf16 matrix pipe.  The fp32 MFMA runs at 1/16 of the bf16 rate, and a
//     16-wide tiling of a 101-column system computes 1.42x the useful flops: at 157 TF that is
//     9.1 ms per Netflix half-iteration against 5.05 ms of HBM time.  Here every
//     gathered fp32 value x is split exactly into three bf16 terms x = h + m + l
//     (round-to-nearest; 8 + 8 + 8 significand bits) and the product of two values is
//     evaluated as hh + hm + mh + mm + hl + lh on v_mfma_f32_16x16x32_bf16 with fp32
//     accumulation: the dropped terms (ml, lm, ll) are below 2^-23 of the product, i.e.
//     below the rounding error of one fp32 fmaf on a sum of two such products.  Every bf16
//     product is exact in fp32.  Error against an fp64 Gram is the same class as the fmaf
//     chain's (tests/test_gpu_parity.py::test_split_gram_error_class); the bit-exact fp32
//     MFMA path stays available (cumf_set_gram_mode / CUMF_ALS_GRAM=exact), and an opt-in 22-bit
//     arithmetic on pre-split f16 pairs (kArithFast, CUMF_ALS_GRAM=fast) halves the matrix-pipe work.
//
// The stage on a PRE-SPLIT gather table (kArithPre, kArithPrePk): als_wave_pre.h.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "als_device.h"
#include "als_lu_blocked.h"
#include "als_internal.h"

namespace cumf {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef int i32x4u __attribute__((ext_vector_type(4), aligned(4)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
typedef __attribute__((address_space(3))) float* lds_float_ptr;  // LDS pointer kept in its own address space (M0 operand)

#ifndef CUMF_ABLATE_STAGE
#define CUMF_ABLATE_STAGE 0
#endif

constexpr int kWaveStage = 32;   // ratings per stage = K of v_mfma_f32_16x16x32_bf16
constexpr int kZeroFloats = 256; // >= 16 * kMaxWaveNB + 16

// Zeros that stand in for "no rating here": ratings past the end of an item gather from
// this row, the pad lanes of the last feature block read it too.
static __device__ __attribute__((aligned(16))) float g_wave_zeros[kZeroFloats];
__device__ __forceinline__ f32x4 mfma_bf16(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0,
                                                 0);
}

__device__ __forceinline__ f32x4 mfma_f16(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// Arithmetic of the Gram pass.  kArithSplit3: exact bf16x3 split, six products (24 significand bits).
// kArithFast: the gather table arrives PRE-SPLIT (presplit_f16x2_kernel, als_kernels.hip): one 32-bit word
// per value = (h, l) f16 pair of 4096 x, x ~ (h + l) / 4096 to 2^-22; three f16 products hh + hl + lh
// (the dropped ll is < 2^-22 of the product), fp32 accumulation, accumulators scaled back by 2^-24.
// kArithPre (round 6): the 24-bit arithmetic of kArithSplit3 -- the same three bf16 planes, the same products, the same
// K slots, bit-identical accumulators -- from a gather table that arrives PRE-SPLIT (presplit_bf16x3_kernel: per row the
// h | m | l planes as 16-bit arrays): the rows are copied into LDS by 16-byte LDS-DMA and the MFMA operands come out of
// ds_read_b64_tr_b16, the 16-bit transposing read of gfx950 -- no split, no pack, no select on the VALU.  For gather
// tables that live in the caches (the Netflix Theta side: X = 7 MB; the hugewiki X side: Theta = 16 MB); an HBM-resident
// table stays fp32 (1.5 x the bytes would cost more than the VALU work saves).  (The kArith* enum: als_internal.h.)
// kArithSplitPk (round 6): the in-kernel split with the last block PACKED, for f % 16 == 0 -- there the last feature block holds
// nothing but the rating slot, and six products per tile of its column (four on its diagonal tile) multiply 15 zero columns.
// The rating is loaded by the lanes of columns 0, 1, 2, split like a feature, and lane c keeps plane c: the packed operand
// [r_h r_m r_l 0 ...] of kArithPrePk -- three products h_I pk + m_I pk + l_I pk per tile (all nine plane products), one (pk pk^T)
// on the diagonal tile, folded back once per item by wave_fold_strip; the gather skips the block (no LDS-DMA, no chunk).
// 65 instead of 80 MFMAs and 32 instead of 40 gathers per stage at f = 64.
constexpr float kFastScale = 4096.0f;             // values must stay below 65504 / 4096 = 15.99 in magnitude
constexpr float kFastUnscale = 1.0f / (4096.0f * 4096.0f);

// (h, l) word of one fp32 value, as presplit_f16x2_kernel makes them (round to nearest even)
__device__ __forceinline__ unsigned fast_word(float x) {
  const float s = x * kFastScale;
  const _Float16 h = (_Float16)s;
  const _Float16 l = (_Float16)(s - (float)h);
  f16x2 w = {h, l};
  return __builtin_bit_cast(unsigned, w);
}

// ----------------------------------------------------------------------------------
// One 32-rating stage in flight: the raw gathered values in the operand layout and its
// column indices.  Planes: the three bf16 terms of a converted stage.
// ----------------------------------------------------------------------------------
template <int NB>
struct WaveStage {
  float raw[NB][8];  // raw[b][e]: feature 16 b + c of rating 8 g + e
  float rv[8];       // rating values (lanes of slot f; zeros elsewhere)
  int idx[8];        // column indices of a stage whose gathers are still to be issued
};
template <int NB, int ARITH = kArithSplit3>
struct Planes {
  u32x4 h[NB], m[NB], l[NB];
};
template <int NB>
struct Planes<NB, kArithFast> {
  u32x4 h[NB], l[NB];
};
// kArithPrePk / kArithSplitPk: the last block as ONE packed operand (GramSchedPk)
template <int NB>
struct Planes<NB, kArithPrePk> {
  u32x4 h[NB], m[NB], l[NB];  // blocks 0 .. NB - 2
  u32x4 pk;                   // the last block, packed
};
template <int NB>
struct Planes<NB, kArithSplitPk> : Planes<NB, kArithPrePk> {};

// Loop-invariant per-lane state of the gather.  FULL forms assume every rating of the stage
// exists (16-byte index / rating loads, no selects); the generic forms clamp the index loads to
// the item, point the ratings past its end at the zero row and zero their rating value.
// PK (kArithSplitPk, f % 16 == 0): the last block holds nothing but the rating -- no chunk of it, the rating in the lanes of
// columns 0, 1, 2.
template <int NB, bool PK = false>
struct WaveGather {
  const char* lane_base;   // gather table + 4 c
  const char* zero_base;   // zero row + 4 c
  const float* val_base;   // val + begin + 8 g in the lanes of slot f, the zero row elsewhere
  const int* idx_base;     // colidx + begin + 8 g
  long long last_off;      // last feature block: byte offset of this lane's load from the row pointer
  unsigned row_bytes;
  int g, len;
#if CUMF_ABLATE
  int dbg;
  unsigned idx_mask;
#endif
  bool is_feat, is_val;    // last feature block: this lane holds a feature / the rating slot
  bool has_val;            // is_val and the item has ratings (an empty row reads zeros instead)

  __device__ __forceinline__ void init(const KernelArgs& a, int f, long long begin, int len_, int lane) {
    const int c = lane & 15;
    g = lane >> 4;
    len = len_;
    row_bytes = (unsigned)f * 4u;
#if CUMF_ABLATE
    if (a.dbg & 8) row_bytes = 0u;  // ablation: every gather hits row 0
    dbg = a.dbg;
    // ablation: the gathers keep their shape (four 64-byte row segments per instruction) but only touch the first
    // 64 / 4096 / 65536 rows of the table (L1- / L2- / MALL-resident at f = 100): profiles/r03/gather_ablation.txt
    idx_mask = (a.dbg & 32) ? 63u : (a.dbg & 64) ? 4095u : (a.dbg & 128) ? 65535u : 0xffffffffu;
#endif
    lane_base = reinterpret_cast<const char*>(a.gather) + 4 * c;
    zero_base = reinterpret_cast<const char*>(g_wave_zeros) + 4 * c;
    const int fi = 16 * (NB - 1) + c;
    is_feat = fi < f;
    is_val = PK ? c < 3 : fi == f;
    // lanes behind the features re-read the start of the row (in bounds) and drop the value
    last_off = is_feat ? 64 * (NB - 1) : -4 * c;
    // A row without ratings still runs ONE stage, on zeros (the accumulators then flow from the stage loop into
    // the solver without a merge with a "no stage" path: that merge cost 41 spilled registers in the LU kernel).
    // Its index / rating loads must not touch colidx / val (begin may be the end of the arrays): they read the
    // zero row; "+ 8 g + 1" because the clamped index forms address the item's last rating at base[-1 - 8 g].
    has_val = is_val && len_ > 0 && a.val != nullptr;  // val == nullptr: no ratings given, the slot reads zeros
    val_base = has_val ? a.val + begin + 8 * g : g_wave_zeros;
    idx_base = len_ > 0 ? a.colidx + begin + 8 * g : reinterpret_cast<const int*>(g_wave_zeros) + 8 * g + 1;
  }

  template <bool FULL>
  __device__ __forceinline__ void load_idx(WaveStage<NB>& st, int s) const {
    const int* p = idx_base + kWaveStage * s;
    if constexpr (FULL) {
      const i32x4u lo = *reinterpret_cast<const i32x4u*>(p);
      const i32x4u hi = *reinterpret_cast<const i32x4u*>(p + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        st.idx[e] = lo[e];
        st.idx[4 + e] = hi[e];
      }
    } else {
      const int last = len - 1 - (kWaveStage * s + 8 * g);  // offset of the item's last rating from p
#pragma unroll
      for (int e = 0; e < 8; ++e) st.idx[e] = p[e < last ? e : last];
    }
  }

  // the rating rides in slot f of the last block (als.cu:750-757 fused into the Gram: column f of
  // the last tile column is sum r * theta = the right-hand side)
  template <bool FULL>
  __device__ __forceinline__ void load_rv(WaveStage<NB>& st, int s) const {
    const float* vp = val_base + (has_val ? kWaveStage * s : 0);
    if constexpr (FULL) {
      const f32x4u lo = *reinterpret_cast<const f32x4u*>(vp);
      const f32x4u hi = *reinterpret_cast<const f32x4u*>(vp + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        st.rv[e] = lo[e];
        st.rv[4 + e] = hi[e];
      }
    } else {
      // ratings past the end of the item read the item's last rating (in bounds) and are then zeroed: their factor
      // rows are the zero row, so the right-hand side never saw them, but entry (f, f) of the augmented Gram --
      // sum r^2, what the fused train SSE starts from (wave_tile_ff) -- would
      const int last = has_val ? len - 1 - (kWaveStage * s + 8 * g) : 7;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float v = vp[e < last ? e : last];
        st.rv[e] = e <= last ? v : 0.f;
      }
    }
  }

  // row pointer (+ 4 c) of rating e of stage s, from st.idx
  template <bool FULL, int E>
  __device__ __forceinline__ const char* row_ptr(const WaveStage<NB>& st, int s) const {
#if CUMF_ABLATE
    const char* row = lane_base + (unsigned long long)((unsigned)st.idx[E] & idx_mask) * row_bytes;
#else
    const char* row = lane_base + (unsigned long long)(unsigned)st.idx[E] * row_bytes;  // v_mad_u64_u32
#endif
    if constexpr (!FULL) {
      const int left = len - (kWaveStage * s + 8 * g);  // ratings of the item from this lane group's first on
      const char* z = zero_base;
      row = (E < left) ? row : z;
    }
    return row;
  }
  // ---- prefetch through LDS: global_load_lds_dword writes lane l's dword to (LDS pointer in M0) +
  // instruction offset + 4 l, so every (rating, feature block) gather of the wave lands as one 256-byte
  // chunk, in flight without holding registers.  Chunk k = e * NB + b at floats [64 k, 64 k + 64).
  template <bool FULL>
  __device__ __forceinline__ void dma_issue(const WaveStage<NB>& st, lds_float_ptr lds, int s) const {
    using gptr = const __attribute__((address_space(1))) void*;
    using lptr = __attribute__((address_space(3))) void*;
    static_for<8>([&](auto ec) {
      constexpr int E = decltype(ec)::value;
      const char* row = row_ptr<FULL, E>(st, s);
      static_for<PK ? NB - 1 : NB>([&](auto bc) {
        constexpr int B = decltype(bc)::value;
        constexpr int k = E * NB + B;
        if constexpr (B + 1 < NB) {
          // the instruction offset (64 B: the block's byte offset in the row) moves BOTH addresses:
          // take it back out of the LDS pointer
          __builtin_amdgcn_global_load_lds((gptr)row, (lptr)(lds + 64 * k - 16 * B), 4, 64 * B, 0);
        } else {
          __builtin_amdgcn_global_load_lds((gptr)(row + last_off), (lptr)(lds + 64 * k), 4, 0, 0);
        }
      });
    });
  }
  // profiling build, switch 16: no gather DMA in the select-free steps (the instances with every block's chunks only)
  __device__ __forceinline__ bool prefetch_dma() const {
#if CUMF_ABLATE
    if constexpr (!PK) return !(dbg & 16);
#endif
    return true;
  }
  // chunk -> registers (after s_waitcnt vmcnt(0))
  __device__ __forceinline__ void dma_read(WaveStage<NB>& st, const float* lds_lane) const {
    static_for<8>([&](auto ec) {
      constexpr int E = decltype(ec)::value;
      static_for<PK ? NB - 1 : NB>([&](auto bc) {
        constexpr int B = decltype(bc)::value;
        st.raw[B][E] = lds_lane[64 * (E * NB + B)];
      });
    });
  }

  // after the loads have landed: the rating / the zero padding into rating E of the last block
  template <int E, int ARITH = kArithSplit3>
  __device__ __forceinline__ void finish_one(WaveStage<NB>& st) const {
    if constexpr (ARITH == kArithFast) {  // the table words are pre-split, the rating is split here
      float w = __builtin_bit_cast(float, fast_word(st.rv[E]));
      asm volatile("" : "+v"(w));  // computed by every lane, then ONE select (a conditional conversion compiles to exec-mask branches)
      st.raw[NB - 1][E] = is_feat ? st.raw[NB - 1][E] : w;
    } else if constexpr (ARITH == kArithSplitPk) {
      st.raw[NB - 1][E] = st.rv[E];  // no feature in the block: the rating (columns 0 .. 2) or zero
    } else
      st.raw[NB - 1][E] = is_feat ? st.raw[NB - 1][E] : st.rv[E];
  }
};

// Exact three-way split x = h + m + l of ratings 2 V, 2 V + 1 of feature block B.  x - h and
// (x - h) - m are exact in fp32 (h carries the leading 8 significand bits of x, m the next 8), and the
// last residual has at most 8 significant bits, so its conversion is exact too.  Cut into six
// micro-steps of 1-3 VALU instructions so that the pipeline can drop one behind every MFMA.
struct SplitState {
  float a, b, ra, rb, ta, tb;
  unsigned H, M;
};
template <int NB, int B, int V, int STEP, class PL>
__device__ __forceinline__ void split_micro(const WaveStage<NB>& st, PL& P, SplitState& x) {
  if constexpr (STEP == 0) {
    x.a = st.raw[B][2 * V];
    x.b = st.raw[B][2 * V + 1];
    x.H = pack_bf16(x.a, x.b);
  } else if constexpr (STEP == 1) {
    x.ra = sub_bf16_lo(x.a, x.H);
  } else if constexpr (STEP == 2) {
    x.rb = sub_bf16_hi(x.b, x.H);
  } else if constexpr (STEP == 3) {
    x.M = pack_bf16(x.ra, x.rb);
  } else if constexpr (STEP == 4) {
    x.ta = sub_bf16_lo(x.ra, x.M);
    x.tb = sub_bf16_hi(x.rb, x.M);
  } else {
    P.h[B][V] = x.H;
    P.m[B][V] = x.M;
    P.l[B][V] = pack_bf16(x.ta, x.tb);
  }
}
template <int NB, int B, int V, class PL>
__device__ __forceinline__ void split_pair(const WaveStage<NB>& st, PL& P) {
  SplitState x;
  static_for<6>([&](auto sc) { split_micro<NB, B, V, decltype(sc)::value>(st, P, x); });
}
// kArithFast: the stage registers hold (h, l) words; the operand words pair two ratings: two v_perm_b32
template <int NB, int B, int V>
__device__ __forceinline__ void split_pair(const WaveStage<NB>& st, Planes<NB, kArithFast>& P) {
  const unsigned wa = __builtin_bit_cast(unsigned, st.raw[B][2 * V]);
  const unsigned wb = __builtin_bit_cast(unsigned, st.raw[B][2 * V + 1]);
  P.h[B][V] = __builtin_amdgcn_perm(wb, wa, 0x05040100u);  // (h of rating 2 V, h of rating 2 V + 1)
  P.l[B][V] = __builtin_amdgcn_perm(wb, wa, 0x07060302u);
}

// tile(I, J) += sum over the 32 ratings of theta[16 I + i] theta[16 J + j] as lh + hl + mm + mh + hm + hh (small terms
// first); kArithFast: lh + hl + hh.
template <int ARITH>
constexpr int gram_products() { return ARITH == kArithFast ? 3 : 6; }

// ----------------------------------------------------------------------------------
// Diagonal tiles at four products instead of six (round 5).  On tile (I, I) both operands come from the same feature
// block, so mh = (hm)^T and lh = (hl)^T: the tile accumulates D + 2 S with D = hh + mm (symmetric) and S = h m^T + h l^T
// -- two MFMAs whose A operand is the h plane with every exponent raised by one (2 h: one v_pk_add_u16 per register,
// exact) -- and ONCE per item, after the last stage, (T + T^T) / 2 = D + S + S^T restores the tile (wave_symmetrise_diag:
// a 16 x 16 transpose through the idle stage buffer).  2 NB of the 6 NT MFMAs of every stage go: 14 of 168 at f = 100.
// The doubled plane lives for three MFMAs: [2h l^T on (I, I)] [an independent tile] [2h m^T on (I, I)].
// Exponent + 1 on a bf16 zero gives 2^-126 -- multiplied by the m / l of a zero value, which are zero; an Inf / NaN still
// reaches the accumulator through hh.  Supported range: finite values with |x| < 2^127 whose leading term h is a
// NORMAL bf16 number or zero -- at biased exponent 0xFE the increment wraps into the Inf / NaN encodings, and a subnormal h is
// not doubled by it; there the diagonal tile's D + 2 S differs from the six-product form of the off-diagonal tiles (factors
// of that size do not occur in ALS: test_split_gram_adversarial_per_entry covers 1e-36 products and nine decades).
// ----------------------------------------------------------------------------------
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32x4 bf16x8_times2(u32x4 v) {
  u32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const unsigned w = v[e];  // through a scalar first: __builtin_bit_cast applied to a vector-element lvalue reads element 0
    r[e] = __builtin_bit_cast(unsigned, (u16x2)(__builtin_bit_cast(u16x2, w) + u16x2{0x0080, 0x0080}));
  }
  return r;
}
// Product kinds: the six plane products of kArithSplit3 in the order a tile takes them (= their product number), the two of a
// diagonal tile's doubled plane, the four against the packed last block (kArithPrePk / kArithSplitPk: GramSchedPk), the three
// f16 products of kArithFast.
enum { kLH = 0, kHL = 1, kMM = 2, kMH = 3, kHM = 4, kHH = 5, kD2L = 6, kD2M = 7, kPL = 8, kPM = 9, kPH = 10, kPP = 11,
       kFLH = 12, kFHL = 13, kFHH = 14 };
template <int ARITH>
constexpr int gram_kind(int prod) { return ARITH == kArithFast ? kFLH + prod : prod; }  // product number -> kind
// THE map from a product kind to MFMA operands: one product of tile (I, J) into its accumulator.
// h2 (kD2L / kD2M only): the doubled plane, two copies used in turn by successive feature blocks (a write straight behind the
// MFMA that reads a register measured safe; what the hardware does need is wait states between the v_pk_add_u16 that WRITES h2
// and the MFMA that reads it -- two for dword 0 / 1 of the operand quad, one for dword 2 / 3:
// tools/probes/mfma_k32_hazard_probe.hip, profiles/r05/mfma_k32_operand_hazard.txt.  The compiler's hazard recogniser supplies
// them (s_nop); that it does is checked on the shipped ISA by
// tests/test_capi_symbols.py::test_k32_mfma_operand_wait_states_in_wave_kernels.)
template <int KIND, int I, int J, class PL>
__device__ __forceinline__ void gram_apply(const PL& P, f32x4& acc, u32x4* h2 = nullptr) {
  if constexpr (KIND == kLH) acc = mfma_bf16(P.l[I], P.h[J], acc);
  if constexpr (KIND == kHL) acc = mfma_bf16(P.h[I], P.l[J], acc);
  if constexpr (KIND == kMM) acc = mfma_bf16(P.m[I], P.m[J], acc);
  if constexpr (KIND == kMH) acc = mfma_bf16(P.m[I], P.h[J], acc);
  if constexpr (KIND == kHM) acc = mfma_bf16(P.h[I], P.m[J], acc);
  if constexpr (KIND == kHH) acc = mfma_bf16(P.h[I], P.h[J], acc);
  if constexpr (KIND == kD2L) {
    h2[I & 1] = bf16x8_times2(P.h[I]);
    acc = mfma_bf16(h2[I & 1], P.l[I], acc);
  }
  if constexpr (KIND == kD2M) acc = mfma_bf16(h2[I & 1], P.m[I], acc);
  if constexpr (KIND == kPL) acc = mfma_bf16(P.l[I], P.pk, acc);
  if constexpr (KIND == kPM) acc = mfma_bf16(P.m[I], P.pk, acc);
  if constexpr (KIND == kPH) acc = mfma_bf16(P.h[I], P.pk, acc);
  if constexpr (KIND == kPP) acc = mfma_bf16(P.pk, P.pk, acc);
  if constexpr (KIND == kFLH) acc = mfma_f16(P.l[I], P.h[J], acc);
  if constexpr (KIND == kFHL) acc = mfma_f16(P.h[I], P.l[J], acc);
  if constexpr (KIND == kFHH) acc = mfma_f16(P.h[I], P.h[J], acc);
}
template <int NB>
struct GramSched {
  static constexpr int NT = NB * (NB + 1) / 2;
  static constexpr int N = 6 * NT - 2 * NB;
  int tile[N], kind[N];
  static constexpr GramSched make();
};
template <int NB>
constexpr GramSched<NB> GramSched<NB>::make() {
  constexpr int NOFF = NT - NB;
  GramSched<NB> s{};
  int off[NOFF > 0 ? NOFF : 1] = {}, dg[NB] = {};
  int no = 0, nd = 0;
  for (int t = 0; t < NT; ++t) {
    if (tile_I<NB>(t) == tile_J<NB>(t)) dg[nd++] = t; else off[no++] = t;
  }
  int n = 0;
  for (int k = 0; k < NOFF; ++k) { s.tile[n] = off[k]; s.kind[n++] = kLH; }
  for (int k = 0; k < NOFF; ++k) { s.tile[n] = off[k]; s.kind[n++] = kHL; }
  int used = 0;  // off-diagonal mm products spent as separators inside the diagonal triples
  for (int I = 0; I < NB; ++I) {
    s.tile[n] = dg[I]; s.kind[n++] = kD2L;
    if (used < NOFF) { s.tile[n] = off[used++]; s.kind[n++] = kMM; }
    s.tile[n] = dg[I]; s.kind[n++] = kD2M;
  }
  for (int k = used; k < NOFF; ++k) { s.tile[n] = off[k]; s.kind[n++] = kMM; }
  for (int I = 0; I < NB; ++I) { s.tile[n] = dg[I]; s.kind[n++] = kMM; }
  for (int k = 0; k < NOFF; ++k) { s.tile[n] = off[k]; s.kind[n++] = kMH; }
  for (int k = 0; k < NOFF; ++k) { s.tile[n] = off[k]; s.kind[n++] = kHM; }
  for (int t = 0; t < NT; ++t) { s.tile[n] = t; s.kind[n++] = kHH; }
  return s;
}
// n-th MFMA of a stage on the schedule SCHED (GramSched, GramSchedPk): consecutive MFMAs hit different accumulators
template <int NB, template <int> class SCHED, int N, class PL>
__device__ __forceinline__ void gram_mfma_sched(const PL& P, f32x4 (&acc)[NB * (NB + 1) / 2], u32x4 (&h2)[2]) {
  constexpr SCHED<NB> S = SCHED<NB>::make();
  constexpr int t = S.tile[N];
  gram_apply<S.kind[N], tile_I<NB>(t), tile_J<NB>(t)>(P, acc[t], h2);
}
// (T + T^T) / 2 on the diagonal tiles, once per item: lane (g, c) register r holds T[4 g + r][c]; every tile goes through
// its own 16 x 17 window of the wave's stage buffer (idle: the last stage prefetches nothing; LDS operations of one wave
// execute in order).  A diagonal entry comes back as itself.
template <int NB>
__device__ __forceinline__ void wave_symmetrise_diag(f32x4 (&acc)[NB * (NB + 1) / 2], float* win, int lane) {
  const int c = lane & 15, g = lane >> 4;
  static_for<NB>([&](auto ic) {
    constexpr int I = decltype(ic)::value;
    constexpr int t = tile_of<NB>(I, I);
    float* w = win + I * 16 * 17;
#pragma unroll
    for (int r = 0; r < 4; ++r) w[(4 * g + r) * 17 + c] = acc[t][r];
  });
  static_for<NB>([&](auto ic) {
    constexpr int I = decltype(ic)::value;
    constexpr int t = tile_of<NB>(I, I);
    const float* w = win + I * 16 * 17;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[t][r] = 0.5f * (acc[t][r] + w[c * 17 + 4 * g + r]);
  });
}

// MFMA schedule of kArithPrePk: as GramSched on the full blocks (six products, four on their diagonal tiles); the last
// block column three products against the packed operand (kPL, kPM, kPH: small terms first), its diagonal tile one (kPP).
// In TWO groups: the tiles among the first HB feature blocks (+ their strip tiles) first -- their operands are the first
// transposing reads to return, so these MFMAs run while the reads of the other blocks are still in flight (the waits are
// the compiler's, per operand); the LDS-DMA of the next stage is issued between the groups, behind the last read.  The
// order of the products of any ONE tile is the same in both groups and as in GramSched.
template <int NB>
struct GramSchedPk {
  static constexpr int FB = NB - 1, NTF = FB * (FB + 1) / 2;
  static constexpr int N = 6 * NTF - 2 * FB + 3 * FB + 1;
  static constexpr int HB = FB >= 4 ? FB / 2 : FB;  // blocks of the first group (all of them for small systems)
  int tile[N], kind[N];
  int n1;  // MFMAs of the first group
  static constexpr GramSchedPk make();
};
template <int NB>
constexpr GramSchedPk<NB> GramSchedPk<NB>::make() {
  GramSchedPk<NB> s{};
  int n = 0;
  for (int grp = 0; grp < 2; ++grp) {
    // tiles of this group: (I, J) with max(I, J) < HB (group 0) or >= HB (group 1); strip tile I with I < HB / >= HB
    auto in = [&](int I, int J) { return ((I > J ? I : J) < HB) == (grp == 0); };
    int off[FB * FB + 1] = {}, dg[FB + 1] = {}, st[FB + 1] = {};
    int no = 0, nd = 0, ns = 0;
    for (int I = 0; I < FB; ++I) {
      if (in(I, I)) { dg[nd++] = I; st[ns++] = tile_of<NB>(I, NB - 1); }
      for (int J = I + 1; J < FB; ++J)
        if (in(I, J)) off[no++] = tile_of<NB>(I, J);
    }
    for (int k = 0; k < no; ++k) { s.tile[n] = off[k]; s.kind[n++] = kLH; }
    for (int k = 0; k < ns; ++k) { s.tile[n] = st[k]; s.kind[n++] = kPL; }
    for (int k = 0; k < no; ++k) { s.tile[n] = off[k]; s.kind[n++] = kHL; }
    int used = 0;  // separators inside the diagonal triples: off-diagonal mm products, then the strip's m products
    for (int k = 0; k < nd; ++k) {
      s.tile[n] = tile_of<NB>(dg[k], dg[k]); s.kind[n++] = kD2L;
      if (used < no) { s.tile[n] = off[used]; s.kind[n++] = kMM; }
      else if (used - no < ns) { s.tile[n] = st[used - no]; s.kind[n++] = kPM; }
      ++used;
      s.tile[n] = tile_of<NB>(dg[k], dg[k]); s.kind[n++] = kD2M;
    }
    for (int k = used; k < no; ++k) { s.tile[n] = off[k]; s.kind[n++] = kMM; }
    for (int k = (used > no ? used - no : 0); k < ns; ++k) { s.tile[n] = st[k]; s.kind[n++] = kPM; }
    for (int k = 0; k < nd; ++k) { s.tile[n] = tile_of<NB>(dg[k], dg[k]); s.kind[n++] = kMM; }
    for (int k = 0; k < no; ++k) { s.tile[n] = off[k]; s.kind[n++] = kMH; }
    for (int k = 0; k < no; ++k) { s.tile[n] = off[k]; s.kind[n++] = kHM; }
    for (int k = 0; k < ns; ++k) { s.tile[n] = st[k]; s.kind[n++] = kPH; }
    for (int k = 0; k < nd; ++k) { s.tile[n] = tile_of<NB>(dg[k], dg[k]); s.kind[n++] = kHH; }
    for (int k = 0; k < no; ++k) { s.tile[n] = off[k]; s.kind[n++] = kHH; }
    if (grp == 0) {
      s.tile[n] = tile_of<NB>(NB - 1, NB - 1); s.kind[n++] = kPP;
      s.n1 = n;
    }
  }
  return s;
}

// kArithPrePk, once per item behind the last stage: the packed column groups of the last block column back into the
// layout every consumer expects (columns 0 .. 4 SP - 1: the strip's features, column 4 SP: the right-hand side, zeros
// behind).  With n = 4 SP:  G[.][j] = S[.][j] + S[.][n + j] + S[.][2 n + j],  G[.][n] = S[.][3 n] + S[.][3 n + 1] + S[.][3 n + 2];
// the diagonal tile (NB - 1, NB - 1) = pk pk^T folds its rows the same way (rows 4 g + r: plane g of feature r, g = 3: the
// rating's three terms) -- two ds_bpermute per register + one for the rating row.
template <int N>
__device__ __forceinline__ float dpp_row_shl(float v) {  // lane c of every 16-lane row reads lane c + N of its row (0 past its end)
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x100 + N, 0xf, 0xf, true));
}
__device__ __forceinline__ float fold_strip_cols(float v, bool sp, int c) {
  const float u = (v + dpp_row_shl<1>(v)) + dpp_row_shl<2>(v);  // lane 3 n: the rating's three terms
  if (sp) {  // wave-uniform
    const float a = (v + dpp_row_shl<4>(v)) + dpp_row_shl<8>(v);
    const float r = dpp_row_shl<8>(u);                          // lane 4 <- lane 12
    return c < 4 ? a : (c == 4 ? r : 0.f);
  }
  return c == 0 ? u : 0.f;
}
template <int NB>
__device__ __forceinline__ void wave_fold_strip(f32x4 (&acc)[NB * (NB + 1) / 2], bool sp, int lane) {
  const int c = lane & 15, g = lane >> 4;
  static_for<NB>([&](auto ic) {
    constexpr int t = tile_of<NB>(decltype(ic)::value, NB - 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[t][r] = fold_strip_cols(acc[t][r], sp, c);
  });
  constexpr int t = tile_of<NB>(NB - 1, NB - 1);
  float w[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) w[r] = acc[t][r];
  const float rt = (w[0] + w[1]) + w[2];  // lane group 3 (SP) / 0 (no strip): the rating row's three terms
  if (sp) {  // wave-uniform
    const float y = bperm(4 * ((lane + 32) & 63), rt);  // lane group 1 <- lane group 3
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float x1 = bperm(4 * ((lane + 16) & 63), w[r]), x2 = bperm(4 * ((lane + 32) & 63), w[r]);
      const float rows = (w[r] + x1) + x2;  // lane group 0: planes h + m + l of feature row r
      acc[t][r] = g == 0 ? rows : ((g == 1 && r == 0) ? y : 0.f);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[t][r] = (g == 0 && r == 0) ? rt : 0.f;
  }
}

// ----------------------------------------------------------------------------------
// One stage, sized for TWO waves per SIMD (<= 256 registers per lane).  A wave cannot hide its own
// VALU work behind its own 16-cycle MFMAs (measured: stage time = MFMA time + VALU time with one
// wave per SIMD, whatever the interleave), so the overlap comes from the partner wave: this
// wave's split burst runs under the partner's MFMA phase and vice versa.  The gather latency
// (~4 000 cycles under load, measured) is covered by prefetching the NEXT stage through LDS
// (global_load_lds: no registers in flight) before the split + MFMAs of this one:
//   wait for the chunks of stage s -> registers -> issue the chunks of stage s + 1 -> split ->
//   6 NT MFMAs.
// (Program order, not issue order: the compiler's scheduler sinks most of the LDS-DMA instructions behind the MFMA burst.
// Round 5 pinned them in front of the split (sched_barrier) and interleaved them with it (sched_group_barrier): no
// gain either way -- X side 6.75-6.87 vs 6.69-6.85 ms, Theta side 10.75-11.06 vs 10.52-10.60, same box,
// profiles/r05/stage_variants_ab.txt -- the partner wave covers the gather latency; the tree keeps the compiler's order.)
// ----------------------------------------------------------------------------------
template <int NB, int PROD, int ARITH>
__device__ __forceinline__ void gram_product(const Planes<NB, ARITH>& P, f32x4 (&acc)[NB * (NB + 1) / 2]) {
  constexpr int NT = NB * (NB + 1) / 2;
  static_for<NT>([&](auto tc) {  // consecutive MFMAs hit different accumulators
    constexpr int t = decltype(tc)::value;
    gram_apply<gram_kind<ARITH>(PROD), tile_I<NB>(t), tile_J<NB>(t)>(P, acc[t]);
  });
}

enum { kStepPartial = 0, kStepFull = 1, kStepLast = 2 };  // prefetch of the step: clamped / select-free / none (last stage of the item)
// The prefetch of one step, once the stage buffer is free: the LDS-DMA of stage s_next (consumes R.idx), its rating values,
// the indices of stage s_idx.  (stage_step_pre and stage_step_pk, als_wave_pre.h, keep blocks of their own on PreGather: routed
// through this function their kernels came out with other instructions.)
template <int KIND, int NB, bool PK>
__device__ __forceinline__ void stage_prefetch(const WaveGather<NB, PK>& wg, WaveStage<NB>& R, lds_float_ptr lds, int s_next,
                                               int s_idx) {
  if constexpr (KIND == kStepFull) {
    if (wg.prefetch_dma()) wg.template dma_issue<true>(R, lds, s_next);
    wg.template load_rv<true>(R, s_next);
    wg.template load_idx<true>(R, s_idx);
  } else if constexpr (KIND == kStepPartial) {
    // the last steps of an item: wave-uniform choices between the select-free and the clamped forms
    // (every step waits for vmcnt(0) anyway, so loads under a uniform branch cost nothing extra)
    const int nfull = wg.len / kWaveStage, nst = (wg.len + kWaveStage - 1) / kWaveStage;
    if (s_next < nfull) {
      wg.template dma_issue<true>(R, lds, s_next);
      wg.template load_rv<true>(R, s_next);
    } else {
      wg.template dma_issue<false>(R, lds, s_next);
      wg.template load_rv<false>(R, s_next);
    }
    if (s_idx < nfull)
      wg.template load_idx<true>(R, s_idx);
    else if (s_idx < nst)
      wg.template load_idx<false>(R, s_idx);
  }
}
// kArithSplitPk: without the last block's gathers and split, with its packed operand; c = lane & 15.
template <int NB, int KIND, int ARITH>
__device__ __forceinline__ void stage_step(const WaveGather<NB, ARITH == kArithSplitPk>& wg, Planes<NB, ARITH>& P, WaveStage<NB>& R,
                                           lds_float_ptr lds, const float* lds_lane, f32x4 (&acc)[NB * (NB + 1) / 2], int s_next,
                                           int s_idx, int c) {
  constexpr bool SPK = ARITH == kArithSplitPk;
  // in flight: chunks + ratings of the stage that is multiplied now, indices of stage s_next
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the LDS-DMA chunks have landed
  wg.dma_read(R, lds_lane);
  static_for<8>([&](auto ec) { wg.template finish_one<decltype(ec)::value, ARITH>(R); });  // consumes R.rv
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the chunks are in registers, the buffer is free
  stage_prefetch<KIND>(wg, R, lds, s_next, s_idx);
  static_for<4 * (SPK ? NB - 1 : NB)>([&](auto uc) { split_pair<NB, decltype(uc)::value / 4, decltype(uc)::value % 4>(R, P); });
  if constexpr (SPK) {
    // the rating: lanes of column 0 keep its h, column 1 its m, column 2 its l (the other columns hold zeros in all three)
    const bool c1 = c == 1, c2 = c == 2;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      unsigned H, M, L;
      split3_pair(R.raw[NB - 1][2 * v], R.raw[NB - 1][2 * v + 1], H, M, L);
      P.pk[v] = c2 ? L : (c1 ? M : H);
    }
  }
  if constexpr (ARITH == kArithSplit3 || SPK) {
    u32x4 h2[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
    if constexpr (SPK)
      static_for<GramSchedPk<NB>::N>([&](auto nc) { gram_mfma_sched<NB, GramSchedPk, decltype(nc)::value>(P, acc, h2); });
    else
      static_for<GramSched<NB>::N>([&](auto nc) { gram_mfma_sched<NB, GramSched, decltype(nc)::value>(P, acc, h2); });
  } else {
    static_for<gram_products<ARITH>()>([&](auto pc) { gram_product<NB, decltype(pc)::value>(P, acc); });
  }
}

}  // namespace cumf
