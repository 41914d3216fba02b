// als_wave_lu.h -- the LU on the accumulators of ONE wave (lu_wave_blocked<NB, FC, PANEL>): every whole row of
// an LU plan at f = 16 .. 111 (als_wave.hip) and the elimination of the dual-form kernel (als_dual.hip).  Nothing waits on
// another wave.  Two panel schemes (LuPanel) over shared pieces -- the negated system (lu_negate_system), block rows in PAIRS
// with bf16 planes and pending rank-32 updates (lu_pending, lu_put_planes), back substitution straight from the tiles
// through a 16-column LDS window (back_substitute_tiles):
//   kLuPanel4   four 4-pivot panels per block row, rank-4 fp32 MFMAs, side rows (NB <= 6, the dual kernel, NB = 7 under
//               CUMF_ALS_LU16=0): the body of lu_wave_blocked;
//   kLuPanel16  sixteen pivots per step, the block row as T N on the bf16 pipe (NB = 7 by default): lu_wave_blocked16.
// The pieces of the panels (lu_prep_step_s, lu16_row_step, the bf16x3 split): als_lu_blocked.h.
#pragma once
#include "als_device.h"
#include "als_lu_blocked.h"
#include "als_wave_gram.h"  // mfma_bf16

namespace cumf {

enum LuPanel { kLuPanel4, kLuPanel16 };

// ----------------------------------------------------------------------------------
// Back substitution U x = y straight from the accumulators of one wave, through a small LDS
// window (16 NB rows x 17 floats = 7.6 KB at NB = 7 instead of the 29 KB packed row store, so
// that eight waves fit a CU).  After the elimination tile (I, J), I <= J, holds U (rows above
// and on the diagonal) in the C/D layout and column f holds y.  Same recurrence as
// back_substitute_zeroed (als_device.h): lane i owns rows i, i + 64, ...; row i is scaled by
// 1 / u_ii (z_i = y_i / u_ii, v_ik = u_ik / u_ii), x_k = z_k; per 16-pivot block column kb the
// tiles (0..kb, kb) are written to the window (entries at and left of the diagonal as zeros) and
// every lane reads the 16 entries of its rows in that block column, one block ahead of their use
// (LDS operations of one wave execute in order: the window is rewritten behind the reads).
// ----------------------------------------------------------------------------------
constexpr int kBsPitch = 17;
// window + pivot reciprocals + 16 zeros + dummy line, then (128-byte aligned) the SIDE ROWS of kLuPanel4: rows 12 .. 15 of
// every tile above the last block row, as rows of W.  The panel-row exchange of lu_prep_step_s (4 lane groups x NB blocks x 16
// columns x 4 rows = 256 NB floats) aliases the window (272 NB floats): the window is written by the back substitution only,
// the exchange is dead by then.
// Side store: tile t = (I, J) in a slot of kSideSlot = 80 floats, row 12 + k, column c at 80 t + skew(I) + 17 k + c with
// skew(I) = 32 I + 12 + 16 (tile_of(I, I) & 1) (a tile's rows reach 14 floats into the next slot: the 32 I keep block rows
// with different skews apart).  ds_read_b32 serves lanes 0 .. 31 / 32 .. 63 in one cycle each when their banks
// (dword address mod 32) differ; the lane of row i reads the window at 17 i + j -- bank 17 i + j -- and the banks of the lanes
// of rows 12 .. 15 (mod 16) are what the side rows must take over: 80 t + skew = 16 (I + J) + 12 (mod 32), so row 12 + k of
// block I sits on bank 12 + 17 k + 16 I + 16 J + j -- its window bank for even J, that of its partner lane (row + 16: the other
// side lane of the group) for odd J.  A first layout with 16-float rows (banks j and j + 16 only: five lanes per bank) cost
// more LDS cycles than the MFMAs it replaced.
constexpr int kSideSlot = 80;
template <int NB>
__host__ __device__ constexpr int wave_lu_side_offset(int f) {
  return (16 * NB * kBsPitch + ((f + 3) & ~3) + 16 + 64 + 31) & ~31;
}
template <int NB>
__host__ __device__ constexpr int wave_lu_side_skew(int I) { return 32 * I + 12 + 16 * (tile_of<NB>(I, I) & 1); }
template <int NB>
__host__ __device__ constexpr int wave_lu_lds_floats(int f) {
  return wave_lu_side_offset<NB>(f) + kSideSlot * (NB * (NB + 1) / 2) + 32 * NB + 32;
}
// Round 6 (side rows): rows 12 .. 15 of the blocks above the last block row are not in the accumulators as rows of -U -- the
// fourth panel of a block row skips its fp32 MFMAs -- but in `side` as rows of W (scaled by 1 / sqrt(u_kk), rdiag holds the
// matching reciprocal): the lanes of those rows read tile (I, kb) of the side store, one slot further per block column,
// instead of the window (layout and banks: wave_lu_side_offset).
template <int NB, int NQ, bool SIDE = true>
__device__ __forceinline__ float back_substitute_tiles(const f32x4 (&acc)[NB * (NB + 1) / 2], float* T,
                                                      const float* rdiag, const float* zpad, const float* side, int f,
                                                      float* __restrict__ x_global, int lane) {
  const int c = lane & 15, g = lane >> 4;
  const int top = f - 1;
  // block column kb -> window
  auto dump = [&](auto kbc) {
    constexpr int kb = decltype(kbc)::value;
    static_for<kb + 1>([&](auto ic) {
      constexpr int I = decltype(ic)::value;
      constexpr int t = tile_of<NB>(I, kb);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[t][r];
        if constexpr (I == kb) v = (c > 4 * g + r) ? v : 0.f;
        T[(16 * I + 4 * g + r) * kBsPitch + c] = v;
      }
    });
  };
  float z[NQ], rdl[NQ];
  const float* rowp[NQ];  // this lane's row in block column kb (walks down with kb for the side rows)
  int step[NQ];           // floats per block column: kSideSlot for a side row, 0 for a row of the window
  int ib[NQ];  // block of this lane's row
  static_for<NQ>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    const int i = lane + 64 * q;
    const int ic = i < f ? i : f - 1;
    const int I = ic >> 4;
    ib[q] = i < f ? I : 1 << 20;  // rows past f never take part
    const bool srow = SIDE && I < NB - 1 && (ic & 15) >= 12;
    const int tII = I * NB - I * (I - 1) / 2;  // tile_of(I, I); tile_of(I, kb) = tII + kb - I
    const float* sp = side + (tII + (NB - 1) - I) * kSideSlot + 32 * I + 12 + 16 * (tII & 1) + 17 * (ic & 3);
    rowp[q] = srow ? sp : T + ic * kBsPitch;
    step[q] = srow ? kSideSlot : 0;
    rdl[q] = i < f ? rdiag[ic] : 0.f;
  });
  float col[2][16][NQ];
  auto issue = [&](auto kbc, auto bufc) {  // called once per block column, kb = NB - 1 first
    constexpr int kb = decltype(kbc)::value, buf = decltype(bufc)::value, Q = kb >> 2;
    const float* base[Q + 1];
    static_for<Q + 1>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      base[q] = (ib[q] > kb) ? zpad : rowp[q];
      rowp[q] -= step[q];
    });
    static_for<16>([&](auto jc) {  // issued in the order they are consumed (LDS returns in order)
      constexpr int j = 15 - decltype(jc)::value;
      static_for<Q + 1>([&](auto qc) { col[buf][j][decltype(qc)::value] = base[decltype(qc)::value][j]; });
    });
  };
  // y sits in column f of the last block column
  dump(std::integral_constant<int, NB - 1>{});
  static_for<NQ>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    z[q] = rowp[q][f - 16 * (NB - 1)] * rdl[q];
  });
  constexpr int NBLK = NB;
  static_for<NBLK>([&](auto bc) {
    constexpr int n = decltype(bc)::value;
    constexpr int kb = NBLK - 1 - n;
    constexpr int buf = n & 1;
    constexpr int Q = kb >> 2;  // pivots of this block live in z[Q]
    if constexpr (Q < NQ) {
      if constexpr (n == 0) issue(std::integral_constant<int, kb>{}, std::integral_constant<int, buf>{});
      if constexpr (kb > 0) {
        dump(std::integral_constant<int, kb - 1>{});
        issue(std::integral_constant<int, kb - 1>{}, std::integral_constant<int, buf ^ 1>{});
      }
      if (16 * kb <= top) {  // uniform: the last block column may hold nothing but y
        static_for<16>([&](auto jc) {
          constexpr int j = 15 - decltype(jc)::value;
          const int k = 16 * kb + j;
          if (k <= top) {  // uniform; only the last block can be short
            const float xk = __builtin_bit_cast(
                float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, z[Q]), k & 63));
            static_for<Q + 1>([&](auto qc) {
              constexpr int q = decltype(qc)::value;
              z[q] = fmaf(-(col[buf][j][q] * rdl[q]), xk, z[q]);
            });
          }
        });
      }
    }
  });
  float ssq = 0.f;  // this lane's share of ||x||^2 (rows past f hold zeros); the fused train SSE wants it
  static_for<NQ>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    if (lane + 64 * q < f) x_global[lane + 64 * q] = z[q];
    ssq = fmaf(z[q], z[q], ssq);
  });
  return ssq;
}

// ----------------------------------------------------------------------------------
// Unpivoted Gaussian elimination of [A | b] on the accumulators of ONE wave + back substitution: the content of
// cublasSgetrfBatched(PivotArray = NULL) + cublasSgetrsBatched (als.cu:77,98 / 146,166).  Panels of four pivots
// p0 .. p0 + 3 (block row Ip, lane group q); rounds 2-3 ran every panel's rank-4 update on all live tiles with fp32 MFMAs
// (lu_wave, and a software-pipelined form of it: profiles/r04/lu_wave_serial_and_pipelined.hip.txt).
// ----------------------------------------------------------------------------------
// n-th tile (row-major) of the part of the upper triangle below block row I0: rows I0 .. NB - 1
template <int NB, int I0>
__host__ __device__ constexpr int lu_trailing_tile(int n) {
  for (int I = I0; I < NB; ++I) {
    if (n < NB - I) return tile_of<NB>(I, I + n);
    n -= NB - I;
  }
  return -1;
}
// product PROD (small terms first, as in the Gram pass) of the rank-16 bf16 update of tile t
template <int NB, int t, int PROD>
__device__ __forceinline__ void lu_trailing_mfma(f32x4 (&acc)[NB * (NB + 1) / 2], const u32x2 (&h)[NB], const u32x2 (&m)[NB],
                                                 const u32x2 (&l)[NB]) {
  constexpr int I = tile_I<NB>(t), J = tile_J<NB>(t);
  if constexpr (PROD == 0) acc[t] = mfma_bf16_k16(l[I], h[J], acc[t]);
  if constexpr (PROD == 1) acc[t] = mfma_bf16_k16(h[I], l[J], acc[t]);
  if constexpr (PROD == 2) acc[t] = mfma_bf16_k16(m[I], m[J], acc[t]);
  if constexpr (PROD == 3) acc[t] = mfma_bf16_k16(m[I], h[J], acc[t]);
  if constexpr (PROD == 4) acc[t] = mfma_bf16_k16(h[I], m[J], acc[t]);
  if constexpr (PROD == 5) acc[t] = mfma_bf16_k16(h[I], h[J], acc[t]);
}

// product PROD of the rank-32 update of tile t by TWO block rows at once (round 6): K slots 0 .. 3 of a lane = the first row's
// four pivots 4 e + g, slots 4 .. 7 = the second row's -- v_mfma_f32_16x16x16_bf16 costs what the K = 32 form costs, so pairing
// the block rows halves the MFMAs of every tile that lies below both (204 instead of 336 per 100 x 100 system)
template <int NB, int t, int PROD>
__device__ __forceinline__ void lu_trailing_mfma32(f32x4 (&acc)[NB * (NB + 1) / 2], const u32x2 (&hA)[NB], const u32x2 (&mA)[NB],
                                                   const u32x2 (&lA)[NB], const u32x2 (&hB)[NB], const u32x2 (&mB)[NB],
                                                   const u32x2 (&lB)[NB]) {
  constexpr int I = tile_I<NB>(t), J = tile_J<NB>(t);
  auto q = [](const u32x2& a, const u32x2& b) { return u32x4{a[0], a[1], b[0], b[1]}; };
  if constexpr (PROD == 0) acc[t] = mfma_bf16(q(lA[I], lB[I]), q(hA[J], hB[J]), acc[t]);
  if constexpr (PROD == 1) acc[t] = mfma_bf16(q(hA[I], hB[I]), q(lA[J], lB[J]), acc[t]);
  if constexpr (PROD == 2) acc[t] = mfma_bf16(q(mA[I], mB[I]), q(mA[J], mB[J]), acc[t]);
  if constexpr (PROD == 3) acc[t] = mfma_bf16(q(mA[I], mB[I]), q(hA[J], hB[J]), acc[t]);
  if constexpr (PROD == 4) acc[t] = mfma_bf16(q(hA[I], hB[I]), q(mA[J], mB[J]), acc[t]);
  if constexpr (PROD == 5) acc[t] = mfma_bf16(q(hA[I], hB[I]), q(hA[J], hB[J]), acc[t]);
}

// the system, negated: -(A + lambda n_u I) (als.cu:545-557 for the diagonal term); lane (g, c)
template <int NB>
__device__ __forceinline__ void lu_negate_system(f32x4 (&acc)[NB * (NB + 1) / 2], float reg, int c, int g) {
  static_for<NB*(NB + 1) / 2>([&](auto tc) {
    constexpr int t = decltype(tc)::value;
    constexpr bool diag = tile_I<NB>(t) == tile_J<NB>(t);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = acc[t][r];
      if constexpr (diag) v = (4 * g + r == c) ? v + reg : v;
      acc[t][r] = -v;
    }
  });
}

// MFMAs PENDING while block row Ip runs (first rows of a pair only): the previous pair's rank-32 update of rows Ip + 1 .. NB - 1
template <int NB, int Ip>
__host__ __device__ constexpr int lu_pending_mfmas() {
  return ((Ip & 1) == 0 && Ip >= 2) ? 6 * ((NB - Ip - 1) * (NB - Ip) / 2) : 0;
}

// bf16 planes of the w of the block row that has just been eliminated (blocks below it): the operands of its rank-16
// update.  The tiles of the NEXT block row get theirs at once (its panels read them); the tiles below that are updated
// ONE MFMA AT A TIME IN FRONT OF THE MICRO-STEPS of the next block row's panels: a bf16 MFMA runs beside the VALU work
// of its own wave only when the two alternate in program order (in-order issue), and the partner wave covers but a
// third of a burst (measured: the update in one burst per block row costs 0.92 ms of the Theta side's 4.6 ms solve).
// Round 6: block rows in PAIRS.  The first row of a pair (Ip even) updates only the second row's tiles at once (rank 16: its
// panels read them); everything below both waits for the second row and then takes ONE rank-32 update with the planes of
// both (A, B) -- the tiles of the next block row at once, the rest one MFMA at a time in front of the micro-steps of the NEXT
// pair's first row.
// The planes hA .. lB: [feature block] of u32x2 {pivots 4 e + g of e = 0, 1 | e = 2, 3}.
// micro-step STEP of the STEPS of block row Ip: pending MFMAs n in [STEP TP / STEPS, (STEP + 1) TP / STEPS), product-major --
// consecutive ones hit different tiles.  The caller closes a micro-step that may carry some with a sched_barrier.
template <int NB, int Ip, int STEP, int STEPS>
__device__ __forceinline__ void lu_pending(f32x4 (&acc)[NB * (NB + 1) / 2], const u32x2 (&hA)[NB], const u32x2 (&mA)[NB],
                                           const u32x2 (&lA)[NB], const u32x2 (&hB)[NB], const u32x2 (&mB)[NB],
                                           const u32x2 (&lB)[NB]) {
  constexpr int TP = lu_pending_mfmas<NB, Ip>(), NTl = TP / 6;
  constexpr int n0 = STEP * TP / STEPS, n1 = (STEP + 1) * TP / STEPS;
  static_for<n1 - n0>([&](auto nc) {
    constexpr int n = n0 + decltype(nc)::value;
    lu_trailing_mfma32<NB, lu_trailing_tile<NB, Ip + 1>(n % NTl), n / NTl>(acc, hA, mA, lA, hB, mB, lB);
  });
}
// the four w (pivots 4 e + g, e = 0 .. 3) of block row Ip at block b > Ip become its planes -- A for the first row of a pair,
// B for the second -- and tile (Ip + 1, b) is updated at once: rank 16 by the first row, rank 32 (both planes) by the second
template <int NB, int Ip, int b>
__device__ __forceinline__ void lu_put_planes(f32x4 (&acc)[NB * (NB + 1) / 2], u32x2 (&hA)[NB], u32x2 (&mA)[NB], u32x2 (&lA)[NB],
                                              u32x2 (&hB)[NB], u32x2 (&mB)[NB], u32x2 (&lB)[NB], float w0, float w1, float w2,
                                              float w3, int dbg) {
#if CUMF_ABLATE
  if (dbg & 1024) return;  // profiling build: 1024 = no trailing update (the planes stay zero)
#endif
  unsigned H0, M0, L0, H1, M1, L1;
  split3_pair(w0, w1, H0, M0, L0);
  split3_pair(w2, w3, H1, M1, L1);
  constexpr int t = tile_of<NB>(Ip + 1, b);
  if constexpr ((Ip & 1) == 0) {
    hA[b] = u32x2{H0, H1};
    mA[b] = u32x2{M0, M1};
    lA[b] = u32x2{L0, L1};
    static_for<6>([&](auto pc) { lu_trailing_mfma<NB, t, decltype(pc)::value>(acc, hA, mA, lA); });
  } else {
    hB[b] = u32x2{H0, H1};
    mB[b] = u32x2{M0, M1};
    lB[b] = u32x2{L0, L1};
    static_for<6>([&](auto pc) { lu_trailing_mfma32<NB, t, decltype(pc)::value>(acc, hA, mA, lA, hB, mB, lB); });
  }
}

#if CUMF_ABLATE
// profiling build, switch 2048: no back substitution (keep the accumulators alive)
template <int NB>
__device__ __forceinline__ float lu_skip_back_substitution(const f32x4 (&acc)[NB * (NB + 1) / 2], int f, float* x_global, int lane) {
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < NB * (NB + 1) / 2; ++t) sum += (acc[t][0] + acc[t][1]) + (acc[t][2] + acc[t][3]);
  if (lane < f) x_global[lane] = sum;
  return sum;
}
#endif

// ---- kLuPanel16: the same elimination with SIXTEEN pivots per step (profiles/lu16/; the default at NB = 7; any NB and a
// run-time f work, NB = 5 and the dual kernel were measured slower with it).  Per block row Ip
//   1. the diagonal tile is eliminated on a copy, read as M[i = c][j = 4 g + r] (the tile is symmetric up to the rounding of
//      its two triangles: the accumulator register is N[4 g + r][c]), by row operations: columns 4 G .. 4 G + 3, the four
//      registers of lane group G, reach all four lane groups with four independent ds_bpermute at pivot step 4 G and take
//      the next three steps as copies (bit for bit what the owner holds; one LDS round trip in the dependency chain per FOUR
//      pivots: profiles/lu16_exchange/), row k with row_newbcast inside the v_fmac (lu16_row_step).  The same operations on the identity
//      leave row c of E = L^-1 in the same layout, which IS the A-operand layout of the MFMA (lane (g, c): T[c][4 g + e]):
//      T = diag(1 / sqrt(u_kk)) E, split exactly into h | m | l in registers (six registers: no LDS image).  A pivot past f
//      eliminates nothing and keeps a unit scale: row f of W stays the Schur complement the fused train SSE reads;
//   2. W(Ip, J) = T N(Ip, J) for every tile of the block row as six bf16 MFMAs (small terms first), N(Ip, J) split in
//      registers (its C/D layout is the B-operand layout).  W = -U / sqrt(u_kk) replaces the tile -- what the side rows were:
//      the back substitution reads every row with the reciprocal -1 / sqrt(u_kk) -- and its split is the trailing operand
//      (K slot (g, e) = pivot 4 g + e, in both operands).
// No panel-row exchange, no fp32 MFMA, no side store; one pending rank-32 MFMA share in front of each pivot step.
template <int NB, int FC>
__device__ __forceinline__ float lu_wave_blocked16(f32x4 (&acc)[NB * (NB + 1) / 2], float* T, int f_rt, float reg,
                                                   float* __restrict__ x_global, int lane, int dbg) {
  const int f = FC ? FC : f_rt;
  const int c = lane & 15, g = (lane >> 4) & 3;
  lu_negate_system<NB>(acc, reg, c, g);
  float* rdiag = T + 16 * NB * kBsPitch;
  float* zpad = rdiag + ((f + 3) & ~3);
  if (lane < 16) zpad[lane] = 0.f;
  u32x2 hA[NB], mA[NB], lA[NB], hB[NB], mB[NB], lB[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) hA[b] = mA[b] = lA[b] = hB[b] = mB[b] = lB[b] = u32x2{0u, 0u};
  static_for<NB>([&](auto ipc) {
    constexpr int Ip = decltype(ipc)::value;
    constexpr int L = NB - Ip;
    constexpr int SD = tile_of<NB>(Ip, Ip);
    // ---- 1. the diagonal tile
    float n[4], e[4], col[4] = {0.f, 0.f, 0.f, 0.f}, rsown = 1.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) n[r] = acc[SD][r], e[r] = (4 * g + r == c) ? 1.0f : 0.f;
    static_for<16>([&](auto kc) {
      constexpr int k = decltype(kc)::value;
      constexpr int p = 16 * Ip + k;
      lu_pending<NB, Ip, k, 16>(acc, hA, mA, lA, hB, mB, lB);
      constexpr bool dyn = FC == 0 && Ip == NB - 1;  // the pivot exists only if p < f (run time)
      if constexpr (FC == 0 || p < FC) {  // a pivot past f eliminates nothing and keeps its row unscaled
        if constexpr ((k & 3) == 0) {  // columns k .. k + 3, the four registers of lane group k >> 2, in every lane group
#if CUMF_ABLATE
          if (dbg & 16384) {  // profiling build: 16384 = no column exchange (every lane group takes its own registers)
#pragma unroll
            for (int r = 0; r < 4; ++r) col[r] = n[r];
          } else
#endif
#pragma unroll
          for (int r = 0; r < 4; ++r) col[r] = bperm(4 * (16 * (k >> 2) + c), n[r]);
        }
        const float colk = col[k & 3];  // M[c][k]
        float rs = __builtin_amdgcn_rsqf(-row_bcast<k>(colk));
        float m = colk * (rs * rs);
        bool act = c > k;
        if constexpr (dyn) act = act && p < f, rs = p < f ? rs : 1.0f;
        m = act ? m : 0.f;
        rsown = (c == k) ? rs : rsown;
        if constexpr (k < 15) lu16_row_step<k>(n, e, col, m);
      }
      if constexpr (lu_pending_mfmas<NB, Ip>() > 0) __builtin_amdgcn_sched_barrier(0);
    });
    if (16 * Ip + c < f) rdiag[16 * Ip + c] = -rsown;  // the rows are rows of W: diagonal -sqrt(u_kk)
    unsigned H0, M0, L0, H1, M1, L1;
    split3_pair(e[0] * rsown, e[1] * rsown, H0, M0, L0);
    split3_pair(e[2] * rsown, e[3] * rsown, H1, M1, L1);
    const u32x2 Th = {H0, H1}, Tm = {M0, M1}, Tl = {L0, L1};
    __builtin_amdgcn_sched_barrier(0);
    // ---- 2. the block row, and the update of the next block row's tiles at once
    static_for<L>([&](auto bc2) {
      constexpr int b = Ip + decltype(bc2)::value;
      constexpr int t = tile_of<NB>(Ip, b);
      split3_pair(acc[t][0], acc[t][1], H0, M0, L0);
      split3_pair(acc[t][2], acc[t][3], H1, M1, L1);
      const u32x2 Nh = {H0, H1}, Nm = {M0, M1}, Nl = {L0, L1};
      f32x4 W = mfma_bf16_k16(Tl, Nh, f32x4{0.f, 0.f, 0.f, 0.f});
      W = mfma_bf16_k16(Th, Nl, W);
      W = mfma_bf16_k16(Tm, Nm, W);
      W = mfma_bf16_k16(Tm, Nh, W);
      W = mfma_bf16_k16(Th, Nm, W);
      W = mfma_bf16_k16(Th, Nh, W);
      acc[t] = W;
      if constexpr (b > Ip) lu_put_planes<NB, Ip, b>(acc, hA, mA, lA, hB, mB, lB, W[0], W[1], W[2], W[3], dbg);
    });
    __builtin_amdgcn_sched_barrier(0);
  });
  __syncthreads();
#if CUMF_ABLATE
  if (dbg & 2048) return lu_skip_back_substitution<NB>(acc, f, x_global, lane);
#endif
  return back_substitute_tiles<NB, (16 * NB + 63) / 64, false>(acc, T, rdiag, zpad, T, f, x_global, lane);
}

// The one-wave LU with the panels of PANEL; returns this lane's share of ||x||^2.  kLuPanel16 hands over to lu_wave_blocked16;
// the body is kLuPanel4: every block row by four 4-pivot panels (lu_prep_step_s, als_lu_blocked.h).  dbg: the profiling
// build's switches (CUMF_ABLATE): 1024 and 2048 act on both schemes, 256, 512 and those of lu_prep_step_s on kLuPanel4 only,
// 16384 on kLuPanel16 only.
// (The two schemes stay two whole functions, kLuPanel4 at this call depth, with plain arrays and pointers: a shared driver,
// a block row as a function of its own, the planes or the window pointers as a struct each compiled some NB = 7 kernel to
// other code -- profiles/lu_skeleton/.)
template <int NB, int FC, LuPanel PANEL>
__device__ __forceinline__ float lu_wave_blocked(f32x4 (&acc)[NB * (NB + 1) / 2], float* T, int f_rt, float reg,
                                                 float* __restrict__ x_global, int lane, int dbg = 0) {
  if constexpr (PANEL == kLuPanel16) return lu_wave_blocked16<NB, FC>(acc, T, f_rt, reg, x_global, lane, dbg);
  const int f = FC ? FC : f_rt;
  LuLaneS ln;
  ln.c = lane & 15;
  ln.kk = (lane >> 4) & 3;
  ln.k1 = ln.kk == 1, ln.k2 = ln.kk == 2, ln.k3 = ln.kk == 3;
  ln.e1c = ln.k1 ? 1.0f : 0.f, ln.e2c = ln.k2 ? 1.0f : 0.f, ln.e3c = ln.k3 ? 1.0f : 0.f;  // unit diagonal of E
  ln.j0 = (lane & 3) == 0, ln.j1 = (lane & 3) >= 1, ln.j2 = (lane & 3) >= 2, ln.j3 = (lane & 3) == 3;
  ln.d1 = (lane & 3) == 1 ? 1.0f : 0.f, ln.d2 = (lane & 3) == 2 ? 1.0f : 0.f;
  lu_negate_system<NB>(acc, reg, ln.c, ln.kk);
  float* rdiag = T + 16 * NB * kBsPitch;
  float* zpad = rdiag + ((f + 3) & ~3);
  if (lane < 16) zpad[lane] = 0.f;
  float* xbuf = T;
  float* side = T + wave_lu_side_offset<NB>(f);
  LuPrepS<NB> s;
  u32x2 hA[NB], mA[NB], lA[NB], hB[NB], mB[NB], lB[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) hA[b] = mA[b] = lA[b] = hB[b] = mB[b] = lB[b] = u32x2{0u, 0u};
  static_for<NB>([&](auto ipc) {
    constexpr int Ip = decltype(ipc)::value;
    constexpr int L = NB - Ip;
    constexpr int S = lu_prep_steps<NB, Ip>();
    float w[4][NB];  // w[e][b]: panel e of this block row at feature block b >= Ip
    static_for<4>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      constexpr int p0 = 16 * Ip + 4 * q;
      constexpr bool last_row = Ip == NB - 1;
      constexpr bool exists_static = !last_row || (FC != 0 && p0 < FC);
      constexpr bool dyn = last_row && FC == 0;            // the panel exists only if p0 < f (run time)
      constexpr bool dynp = (last_row && (FC & 3) != 0) || dyn;  // ... and may be short (a compile-time f that is no multiple of 4 too)
      auto panel = [&]() {
        float wm = 0.f;
#if CUMF_ABLATE
        // profiling build: 256 = no panel preparation (constants instead), 512 = no fp32 MFMAs
        if (dbg & 256) {
          static_for<L>([&](auto bc2) { w[q][Ip + decltype(bc2)::value] = acc[tile_of<NB>(Ip, Ip + decltype(bc2)::value)][q]; });
          wm = w[q][Ip];
        } else
#endif
        static_for<S>([&](auto sc) {
          constexpr int i = decltype(sc)::value;
          lu_pending<NB, Ip, q * S + i, 4 * S>(acc, hA, mA, lA, hB, mB, lB);
          lu_prep_step_s<NB, Ip, q, dynp, i>(acc, s, w[q], wm, rdiag, xbuf, f, ln, dbg);
          if constexpr (lu_pending_mfmas<NB, Ip>() > 0) __builtin_amdgcn_sched_barrier(0);
        });
        if constexpr (q == 3 && !last_row) {
          // Round 6: the fourth panel's update of the block row would only finish its own rows 13 .. 15 for the back
          // substitution (no later panel reads this block row) -- and v_mfma_f32_16x16x4_f32 holds the SIMD for 36 cycles,
          // nothing issues beside it.  Those rows are kept as rows of W instead (lane group kk = row 12 + kk; zeros at and left
          // of the diagonal: wm), one ds_write_b32 per tile; back_substitute_tiles reads them from there.  82 instead of 109
          // fp32 MFMAs per 100 x 100 system.
          static_for<L>([&](auto bc2) {
            constexpr int b = Ip + decltype(bc2)::value;
            side[tile_of<NB>(Ip, b) * kSideSlot + wave_lu_side_skew<NB>(Ip) + 17 * ln.kk + ln.c] = b == Ip ? wm : w[q][b];
          });
        } else {
          // the block row's own tiles: what its next panel reads (and the rows the back substitution reads later)
#if CUMF_ABLATE
          if (!(dbg & 512))
#endif
          static_for<L>([&](auto bc2) {
            constexpr int b = Ip + decltype(bc2)::value;
            constexpr int t = tile_of<NB>(Ip, b);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wm, w[q][b], acc[t], 0, 0, 0);
          });
        }
        __builtin_amdgcn_sched_barrier(0);  // no instruction motion across panels (lu_wave: hoisted broadcasts spill)
      };
      if constexpr (exists_static) {
        panel();
      } else if constexpr (dyn) {
        if (p0 < f) panel();  // wave-uniform
      }
    });
    if constexpr (L > 1) {
      // planes of this block row's w and the tiles of block row Ip + 1, block by block as the planes appear
      static_for<L - 1>([&](auto bc2) {
        constexpr int b = Ip + 1 + decltype(bc2)::value;
        lu_put_planes<NB, Ip, b>(acc, hA, mA, lA, hB, mB, lB, w[0][b], w[1][b], w[2][b], w[3][b], dbg);
      });
      __builtin_amdgcn_sched_barrier(0);
    }
  });
  __syncthreads();  // one wave: orders the rdiag writes before the reads below
#if CUMF_ABLATE
  if (dbg & 2048) return lu_skip_back_substitution<NB>(acc, f, x_global, lane);
#endif
  return back_substitute_tiles<NB, (16 * NB + 63) / 64>(acc, T, rdiag, zpad, side, f, x_global, lane);
}

}  // namespace cumf
