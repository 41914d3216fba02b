// als_wave_solve.h -- what the wave kernels (als_wave.hip) do with a finished tile set: the tile epilogues, the LU and the
// CG on the accumulators, the fused train SSE.
//
//   * LU on the accumulators of the one wave (lu_wave_blocked), per block row: four 4-pivot panels -- the
//     4 x 4 pivot block eliminated where it sits by DPP quad broadcasts, the panel's raw rows to the other lane groups
//     through LDS (every lane stores the four rows it holds of a block as ONE 16-byte word and loads the four rows of the
//     panel's lane group at its column with one 16-byte load), one rank-4 v_mfma_f32_16x16x4_f32 per tile of the block row
//     itself (the elimination of lu_solve_mfma, als_lu_wg.h) -- then the trailing update on the bf16 pipe (lu_trailing_mfma*).
//     The fourth panel of a block row skips its fp32 MFMAs and leaves rows 12 .. 15 as SIDE ROWS in LDS.  Nothing waits on
//     another wave.  Back substitution straight from the tiles through a 16-column LDS window (back_substitute_tiles).
//     NB = 7 eliminates sixteen pivots per step instead (lu_wave_blocked16): the diagonal tile once per block row by DPP row
//     broadcasts, the block row as T N on the bf16 pipe -- no panel-row exchange, no fp32 MFMA, no side rows.
//   * CG on the accumulators (cg_wave_core): vectors in a column layout, the mat-vec on the upper
//     tiles with DPP / ds_bpermute reductions, 1, 2 or 4 waves per system.
#pragma once
#include "als_wave_gram.h"

namespace cumf {

#if CUMF_ABLATE
// profiling build, switch 65536: how many CG iterations (mat-vecs behind the initial residual) the rows actually ran before
// ||r||^2 < 1e-4 ended the loop (cg.cu:195) -- bin k = rows that ran k iterations (cumf_debug_cg_histogram)
static __device__ __attribute__((unused)) unsigned long long g_cg_hist[16];
#endif

// ----------------------------------------------------------------------------------
// Epilogues on the full tile set of one wave (same element layout as als_kernels.hip).
// ----------------------------------------------------------------------------------
template <int NB>
__device__ __forceinline__ void wave_tiles_to_partial(const f32x4 (&acc)[NB * (NB + 1) / 2], float* __restrict__ part,
                                                      int lane) {
  static_for<NB*(NB + 1) / 2>([&](auto tc) {
    constexpr int t = decltype(tc)::value;
#pragma unroll
    for (int r = 0; r < 4; ++r) part[((size_t)t * 4 + r) * 64 + lane] = acc[t][r];
  });
}

// row-major f x f Gram, both triangles, lambda * n on the diagonal (als.cu:545-566) + RHS
template <int NB, typename T>
__device__ __forceinline__ void wave_tiles_to_global(const f32x4 (&acc)[NB * (NB + 1) / 2], T* __restrict__ tt,
                                                     float* __restrict__ rhs, int f, float reg, int lane,
                                                     bool packed = false) {
  const int c = lane & 15, kk = lane >> 4;
  static_for<NB*(NB + 1) / 2>([&](auto tc) {
    constexpr int t = decltype(tc)::value;
    constexpr int I = tile_I<NB>(t), J = tile_J<NB>(t);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * I + 4 * kk + r, j = 16 * J + c;
      float v = acc[t][r];
      if (i < f && j < f) {
        if (i == j) v += reg;
        // both triangles from ONE accumulator entry (als.h:39-143 writes tt[i][j] and tt[j][i] from the same
        // temp): inside a diagonal tile the split products reach (i, j) and (j, i) in different orders, so
        // only the upper entry is used there
        if (I != J || i <= j) {
          if (packed) {  // row i keeps columns i .. f - 1 (cumf_get_hermitian_packed)
            tt[(size_t)i * f - (size_t)(i * (i - 1) / 2) + (j - i)] = (T)v;
          } else {
            tt[(size_t)i * f + j] = (T)v;  // T = _Float16: fp16 Gram storage (als.cu:335-441), round to nearest even
            if (i != j) tt[(size_t)j * f + i] = (T)v;
          }
        }
      } else if (i < f && j == f && rhs != nullptr) {
        rhs[i] = v;
      }
    }
  });
}

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
// window + pivot reciprocals + 16 zeros + dummy line, then (128-byte aligned) the SIDE ROWS of lu_wave_blocked: rows 12 .. 15 of
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
// Train SSE of one row for free (round 4; als.cu:191-219 + 979-991 folded into the Theta update).  The rating rides in
// slot f of the gathered rows, so the Gram pass has also accumulated entry (f, f) of the augmented matrix
// [Theta r]^T [Theta r]: S = sum r^2.  With G = sum x x^T, b = sum r x, A = G + reg I (reg = lambda n):
//   sum_u (r - x_u . t)^2 = S - 2 t.b + t^T G t                                   for ANY t;
//   LU:  the elimination treats row / column f like every other trailing row, so entry (f, f) ends as the Schur
//        complement S + reg - b^T A^-1 b (the diagonal got reg everywhere, slot f included); with A t = b this is
//        S + reg - t.b, and t^T G t = t.b - reg |t|^2, hence SSE = (f, f) - reg (1 + |t|^2);
//   CG:  the tiles are untouched; with the recursive residual r = b - A t:  t^T G t = t.b - t.r - reg |t|^2, hence
//        SSE = S - t.b - t.r - reg |t|^2  (three dot products on vectors the solver holds anyway).
// No rating and no factor row is read again.  One fp64 atomic per row into kSseBins bins (the reference's own
// error bins, als.cu:216, hold fp32 partial sums); rows without ratings contribute nothing.
// ----------------------------------------------------------------------------------
__device__ __forceinline__ void wave_sse_add(double* bins, double sse, int rowlen, int lane) {
  if (lane == 0 && rowlen > 0) atomicAdd(bins + (blockIdx.x & (kSseBins - 1)), sse);
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

// The same elimination with SIXTEEN pivots per step (profiles/lu16/; the default at NB = 7, CUMF_ALS_LU16=0: the four-pivot
// panels of lu_wave_blocked; any NB and a run-time f work, NB = 5 and the dual kernel were measured slower with it).  Per
// block row Ip
//   1. the diagonal tile is eliminated on a copy, read as M[i = c][j = 4 g + r] (the tile is symmetric up to the rounding of
//      its two triangles: the accumulator register is N[4 g + r][c]), by row operations: column k reaches all four lane groups
//      with one ds_bpermute, row k with row_newbcast inside the v_fmac (lu16_row_step).  The same operations on the identity
//      leave row c of E = L^-1 in the same layout, which IS the A-operand layout of the MFMA (lane (g, c): T[c][4 g + e]):
//      T = diag(1 / sqrt(u_kk)) E, split exactly into h | m | l in registers (six registers: no LDS image).  A pivot past f
//      eliminates nothing and keeps a unit scale: row f of W stays the Schur complement the fused train SSE reads;
//   2. W(Ip, J) = T N(Ip, J) for every tile of the block row as six bf16 MFMAs (small terms first), N(Ip, J) split in
//      registers (its C/D layout is the B-operand layout).  W = -U / sqrt(u_kk) replaces the tile -- what the side rows were:
//      the back substitution reads every row with the reciprocal -1 / sqrt(u_kk) -- and its split is the trailing operand
//      (K slot (g, e) = pivot 4 g + e, in both operands).
// No panel-row exchange, no fp32 MFMA, no side store; pairs, pending rank-32 updates (one in front of each pivot step) and the
// back substitution as in lu_wave_blocked.
template <int NB, int FC>
__device__ __forceinline__ float lu_wave_blocked16(f32x4 (&acc)[NB * (NB + 1) / 2], float* T, int f_rt, float reg,
                                                   float* __restrict__ x_global, int lane) {
  constexpr int NT = NB * (NB + 1) / 2;
  const int f = FC ? FC : f_rt;
  const int c = lane & 15, g = (lane >> 4) & 3;
  static_for<NT>([&](auto tc) {
    constexpr int t = decltype(tc)::value;
    constexpr bool diag = tile_I<NB>(t) == tile_J<NB>(t);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = acc[t][r];
      if constexpr (diag) v = (4 * g + r == c) ? v + reg : v;
      acc[t][r] = -v;
    }
  });
  float* rdiag = T + 16 * NB * kBsPitch;
  float* zpad = rdiag + ((f + 3) & ~3);
  if (lane < 16) zpad[lane] = 0.f;
  auto bperm = [](int addr, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addr, __builtin_bit_cast(int, v)));
  };
  u32x2 hA[NB], mA[NB], lA[NB], hB[NB], mB[NB], lB[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) hA[b] = mA[b] = lA[b] = hB[b] = mB[b] = lB[b] = u32x2{0u, 0u};
  static_for<NB>([&](auto ipc) {
    constexpr int Ip = decltype(ipc)::value;
    constexpr int L = NB - Ip;
    constexpr bool FIRST = (Ip & 1) == 0;
    constexpr int NTl = (FIRST && Ip >= 2) ? (L - 1) * L / 2 : 0;
    constexpr int TP = 6 * NTl;
    constexpr int SD = tile_of<NB>(Ip, Ip);
    // ---- 1. the diagonal tile
    float n[4], e[4], rsown = 1.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) n[r] = acc[SD][r], e[r] = (4 * g + r == c) ? 1.0f : 0.f;
    static_for<16>([&](auto kc) {
      constexpr int k = decltype(kc)::value;
      constexpr int p = 16 * Ip + k;
      constexpr int n0 = k * TP / 16, n1 = (k + 1) * TP / 16;
      static_for<n1 - n0>([&](auto nc) {
        constexpr int nn = n0 + decltype(nc)::value;
        lu_trailing_mfma32<NB, lu_trailing_tile<NB, Ip + 1>(nn % NTl), nn / NTl>(acc, hA, mA, lA, hB, mB, lB);
      });
      constexpr bool dyn = FC == 0 && Ip == NB - 1;  // the pivot exists only if p < f (run time)
      if constexpr (FC == 0 || p < FC) {  // a pivot past f eliminates nothing and keeps its row unscaled
        const float colk = bperm(4 * (16 * (k >> 2) + c), n[k & 3]);  // M[c][k], in every lane group
        float rs = __builtin_amdgcn_rsqf(-row_bcast<k>(colk));
        float m = colk * (rs * rs);
        bool act = c > k;
        if constexpr (dyn) act = act && p < f, rs = p < f ? rs : 1.0f;
        m = act ? m : 0.f;
        rsown = (c == k) ? rs : rsown;
        if constexpr (k < 15) lu16_row_step<k>(n, e, m);
      }
      if constexpr (TP > 0) __builtin_amdgcn_sched_barrier(0);
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
      if constexpr (b > Ip) {
        split3_pair(W[0], W[1], H0, M0, L0);
        split3_pair(W[2], W[3], H1, M1, L1);
        constexpr int tn = tile_of<NB>(Ip + 1, b);
        if constexpr (FIRST) {
          hA[b] = u32x2{H0, H1};
          mA[b] = u32x2{M0, M1};
          lA[b] = u32x2{L0, L1};
          static_for<6>([&](auto pc) { lu_trailing_mfma<NB, tn, decltype(pc)::value>(acc, hA, mA, lA); });
        } else {
          hB[b] = u32x2{H0, H1};
          mB[b] = u32x2{M0, M1};
          lB[b] = u32x2{L0, L1};
          static_for<6>([&](auto pc) { lu_trailing_mfma32<NB, tn, decltype(pc)::value>(acc, hA, mA, lA, hB, mB, lB); });
        }
      }
    });
    __builtin_amdgcn_sched_barrier(0);
  });
  __syncthreads();
  return back_substitute_tiles<NB, (16 * NB + 63) / 64, false>(acc, T, rdiag, zpad, T, f, x_global, lane);
}
// P16: the sixteen-pivot panel scheme (lu_wave_blocked16) in place of the four-pivot panels below
template <int NB, int FC, bool P16 = false>
__device__ __forceinline__ float lu_wave_blocked(f32x4 (&acc)[NB * (NB + 1) / 2], float* T, int f_rt, float reg,
                                                 float* __restrict__ x_global, int lane, int dbg = 0) {
  if constexpr (P16) return lu_wave_blocked16<NB, FC>(acc, T, f_rt, reg, x_global, lane);
  constexpr int NT = NB * (NB + 1) / 2;
  const int f = FC ? FC : f_rt;
  LuLaneS ln;
  ln.c = lane & 15;
  ln.kk = (lane >> 4) & 3;
  ln.k1 = ln.kk == 1, ln.k2 = ln.kk == 2, ln.k3 = ln.kk == 3;
  ln.e1c = ln.k1 ? 1.0f : 0.f, ln.e2c = ln.k2 ? 1.0f : 0.f, ln.e3c = ln.k3 ? 1.0f : 0.f;  // unit diagonal of E
  ln.j0 = (lane & 3) == 0, ln.j1 = (lane & 3) >= 1, ln.j2 = (lane & 3) >= 2, ln.j3 = (lane & 3) == 3;
  ln.d1 = (lane & 3) == 1 ? 1.0f : 0.f, ln.d2 = (lane & 3) == 2 ? 1.0f : 0.f;
  // the system, negated: -(A + lambda n_u I) (als.cu:545-557 for the diagonal term)
  static_for<NT>([&](auto tc) {
    constexpr int t = decltype(tc)::value;
    constexpr bool diag = tile_I<NB>(t) == tile_J<NB>(t);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = acc[t][r];
      if constexpr (diag) v = (4 * ln.kk + r == ln.c) ? v + reg : v;
      acc[t][r] = -v;
    }
  });
  float* rdiag = T + 16 * NB * kBsPitch;  // pivot reciprocals, then 16 zeros (rows outside a pivot block read these)
  float* zpad = rdiag + ((f + 3) & ~3);
  if (lane < 16) zpad[lane] = 0.f;
  float* xbuf = T;  // panel-row exchange: [lane group 4][block NB][column 16][row 4], in the (still unused) window
  float* side = T + wave_lu_side_offset<NB>(f);  // rows 12 .. 15 of the tiles above the last block row, as rows of W

  LuPrepS<NB> s;
  // bf16 planes of the w of the block row that has just been eliminated (blocks below it): the operands of its rank-16
  // update.  The tiles of the NEXT block row get theirs at once (its panels read them); the tiles below that are updated
  // ONE MFMA AT A TIME IN FRONT OF THE MICRO-STEPS of the next block row's panels: a bf16 MFMA runs beside the VALU work
  // of its own wave only when the two alternate in program order (in-order issue), and the partner wave covers but a
  // third of a burst (measured: the update in one burst per block row costs 0.92 ms of the Theta side's 4.6 ms solve).
  // Round 6: block rows in PAIRS.  The first row of a pair (Ip even) updates only the second row's tiles at once (rank 16: its
  // panels read them); everything below both waits for the second row and then takes ONE rank-32 update with the planes of
  // both (A, B) -- the tiles of the next block row at once, the rest one MFMA at a time in front of the micro-steps of the NEXT
  // pair's first row.
  u32x2 hA[NB], mA[NB], lA[NB], hB[NB], mB[NB], lB[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) hA[b] = mA[b] = lA[b] = hB[b] = mB[b] = lB[b] = u32x2{0u, 0u};
  static_for<NB>([&](auto ipc) {
    constexpr int Ip = decltype(ipc)::value;
    constexpr int L = NB - Ip;
    constexpr bool FIRST = (Ip & 1) == 0;
    // pending (first rows only): the previous pair's rank-32 update of the tiles below block row Ip
    constexpr int NTl = (FIRST && Ip >= 2) ? (L - 1) * L / 2 : 0;  // tiles of rows Ip + 1 .. NB - 1
    constexpr int TP = 6 * NTl;
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
          constexpr int gs = q * S + i;  // micro-step of the block row
          // pending MFMAs n in [gs TP / 4S, (gs + 1) TP / 4S): product-major, consecutive ones hit different tiles
          constexpr int n0 = gs * TP / (4 * S), n1 = (gs + 1) * TP / (4 * S);
          static_for<n1 - n0>([&](auto nc) {
            constexpr int n = n0 + decltype(nc)::value;
            lu_trailing_mfma32<NB, lu_trailing_tile<NB, Ip + 1>(n % NTl), n / NTl>(acc, hA, mA, lA, hB, mB, lB);
          });
#if CUMF_ABLATE
          lu_prep_step_s<NB, Ip, q, dynp, i>(acc, s, w[q], wm, rdiag, xbuf, f, ln, dbg);
#else
          lu_prep_step_s<NB, Ip, q, dynp, i>(acc, s, w[q], wm, rdiag, xbuf, f, ln);
#endif
          if constexpr (TP > 0) __builtin_amdgcn_sched_barrier(0);
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
#if CUMF_ABLATE
    if (!(dbg & 1024))  // profiling build: 1024 = no trailing update
#endif
    if constexpr (L > 1) {
      // planes of this block row's w; the tiles of block row Ip + 1 at once, block by block as the planes appear: rank 16 by
      // the first row of a pair, rank 32 (both rows' planes) by the second
      static_for<L - 1>([&](auto bc2) {
        constexpr int b = Ip + 1 + decltype(bc2)::value;
        unsigned H0, M0, L0, H1, M1, L1;
        split3_pair(w[0][b], w[1][b], H0, M0, L0);
        split3_pair(w[2][b], w[3][b], H1, M1, L1);
        constexpr int t = tile_of<NB>(Ip + 1, b);
        if constexpr (FIRST) {
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
      });
      __builtin_amdgcn_sched_barrier(0);
    }
  });
  __syncthreads();  // one wave: orders the rdiag writes before the reads below
#if CUMF_ABLATE
  if (dbg & 2048) {  // profiling build: no back substitution
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) sum += (acc[t][0] + acc[t][1]) + (acc[t][2] + acc[t][3]);
    if (lane < f) x_global[lane] = sum;
    return sum;
  }
#endif
  return back_substitute_tiles<NB, (16 * NB + 63) / 64>(acc, T, rdiag, zpad, side, f, x_global, lane);
}

// ----------------------------------------------------------------------------------
// Conjugate gradient on dumped tiles (cg.cu:36-231: warm start, r = b - A x, <= cg_iters iterations,
// stop when ||r||^2 < 1e-4), NW waves per system, wave W holding the tiles t % NW == W in registers.
// Vectors live in "column layout": one register per 16-feature block, lane (g, c) = element
// 16 J + c, replicated over the four lane groups g; every wave keeps all vectors and performs the
// vector updates and dot products redundantly (identical instruction sequences on identical data:
// alpha / beta / the exit test are uniform without communication).  Mat-vec y = A v on a tile
// T = T(I, J), I <= J, in the C/D layout (lane (g, c), register r = T[4 g + r][c]):
//   (1) y_I[4 g + r] += sum_c T[r][c] v_J[c]        4 FMAs, then a 16-lane DPP reduction per (I, r)
//   (2) y_J[c]       += sum_{g, r} T[r][c] v_I[4 g + r]   (I < J: the mirrored half)   4 FMAs with v_I in
//       "row layout" (ds_bpermute from the column layout), then a 4-lane-group reduction per J
// and (1)'s result is brought back to the column layout with 3 selects + 1 ds_bpermute per block.
// NW > 1: the partial y of the waves go through LDS, one workgroup barrier pair per mat-vec.
// Dot products: per-lane FMAs over the blocks + the 16-lane DPP reduction (fixed order), in place of
// the reference's order-dependent shared-memory atomics (device_utilities.h:36-48).
// ----------------------------------------------------------------------------------
__device__ __forceinline__ float row16_sum(float v) {  // all-reduce over the 16 lanes of a DPP row
  v += dpp_term<0xB1, 0xf>(v);   // quad_perm [1,0,3,2]
  v += dpp_term<0x4E, 0xf>(v);   // quad_perm [2,3,0,1]
  v += dpp_term<0x141, 0xf>(v);  // row_half_mirror
  v += dpp_term<0x140, 0xf>(v);  // row_mirror
  return v;
}

// Sums of FOUR registers over the 16 lanes of a DPP row, transposed: every lane c ends with the full sum of
// register c & 3.  11 instructions instead of 4 x row16_sum = 16, and the result is already where the
// row -> column layout change wants it (lane (g, c) holds row 4 g + (c & 3) of the block).
//   xor 1: lanes keep the register of their parity and send the other one  (4 selects + 2 adds)
//   xor 2: the same on the two pair sums                                      (2 selects + 1 add)
//   the four quads of the row hold the same register in the same position: row_ror 4, row_ror 8 (2 adds)
__device__ __forceinline__ float row16_sum4_transposed(float r0, float r1, float r2, float r3, bool c1, bool c2) {
  const float keep01 = c1 ? r1 : r0, send01 = c1 ? r0 : r1;
  const float keep23 = c1 ? r3 : r2, send23 = c1 ? r2 : r3;
  const float t01 = keep01 + dpp_term<0xB1, 0xf>(send01);  // quad_perm [1,0,3,2]
  const float t23 = keep23 + dpp_term<0xB1, 0xf>(send23);
  const float keep = c2 ? t23 : t01, send = c2 ? t01 : t23;
  float w = keep + dpp_term<0x4E, 0xf>(send);  // quad_perm [2,3,0,1]
  w += dpp_term<0x124, 0xf>(w);                // row_ror:4
  w += dpp_term<0x128, 0xf>(w);                // row_ror:8
  return w;
}
// Two FMAs on a register pair, as two scalar v_fma_f32.  Round 3 saw wrong CG mat-vecs (1-4 % of the long Netflix X rows, a
// different set every run) in a build whose compiler had formed v_pk_fma_f32 here (profiles/r03/pk_fma_bisect.txt) and
// kept packed fp32 math out ever since (-fno-slp-vectorize; tests/test_capi_symbols.py disassembles the objects).  Round 4
// looked again: a standalone probe (tools/probes/pk_fma_probe.hip: 3e12 packed FMAs feeding DPP reductions and ds_bpermute
// beside bf16 and fp32 MFMA waves, against scalar FMAs: 0 mismatches) and this very CG with fma2 spelled as ONE inline-asm
// v_pk_fma_f32 (full-size oracle rows green three times, RMSE identical to 1e-16, profiles/r04/pk_fma_cg_ab.txt) are
// clean -- the instruction is not at fault, that build's generated code was -- and the packed CG is 5 % SLOWER (the packed
// FMA issues at half rate and needs aligned register pairs): the scalar form stays, for speed.
__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) {
  return f32x2{fmaf(a[0], b[0], c[0]), fmaf(a[1], b[1], c[1])};
}

template <int NB, int NW, int W, int I>
__host__ __device__ constexpr bool cg_row_has_offdiag() {
  for (int J = I + 1; J < NB; ++J)
    if (tile_of<NB>(I, J) % NW == W) return true;
  return false;
}
template <int NB, int NW, int W, int I>
__host__ __device__ constexpr bool cg_row_has_any() {
  for (int J = I; J < NB; ++J)
    if (tile_of<NB>(I, J) % NW == W) return true;
  return false;
}

template <int NB, int NW, int W>
__device__ __forceinline__ void cg_wave_core(f32x4 (&T)[(NB * (NB + 1) / 2 + NW - 1) / NW], float* smem,
                                             const KernelArgs& a, int f, int row, int rowlen, int lane) {
  const int c = lane & 15, g = lane >> 4;
  auto bperm = [](int addr, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addr, __builtin_bit_cast(int, v)));
  };
  const float reg = (float)rowlen * a.lambda;  // lambda * n_u on the diagonal (als.cu:545-557)
  static_for<NB>([&](auto ic) {
    constexpr int t = tile_of<NB>(decltype(ic)::value, decltype(ic)::value);
    if constexpr (t % NW == W) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float d = T[t / NW][r] + reg;
        T[t / NW][r] = (4 * g + r == c) ? d : T[t / NW][r];
      }
    }
  });
  bool live[NB];  // this lane's element of block J exists (16 J + c < f)
  static_for<NB>([&](auto jc) { live[decltype(jc)::value] = 16 * decltype(jc)::value + c < f; });
  float* xch = smem;  // NW > 1: [wave][NB][16] partial vectors
  const int sel_addr = 4 * (16 * (c >> 2) + c);  // lane (c >> 2, c): holds element c of a row-layout block after (1)
  const int row_addr = 4 * (20 * g);             // + 4 r: lane (g, 4 g + r) holds v[16 I + 4 g + r] in the column layout
  // row layout (lanes of group g, registers r: element 4 g + r, the same in all 16 lanes) -> column layout
  const bool cr1 = (c & 3) == 1, cr2 = (c & 3) == 2, cr3 = (c & 3) == 3;
  auto to_col = [&](const float (&R)[4]) {
    float w = R[0];  // flat selects (v_cndmask): a nested ?: becomes exec-mask branches
    w = cr1 ? R[1] : w;
    w = cr2 ? R[2] : w;
    w = cr3 ? R[3] : w;
    return bperm(sel_addr, w);
  };
  // sum of the waves' partial column-layout vectors (NW > 1)
  auto combine = [&](float (&y)[NB]) {
    if constexpr (NW > 1) {
      __syncthreads();  // the previous exchange has been read
      if (g == 0) {
        static_for<NB>([&](auto jc) { xch[(W * NB + decltype(jc)::value) * 16 + c] = y[decltype(jc)::value]; });
      }
      __syncthreads();
      static_for<NB>([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        float t = 0.f;
        static_for<NW>([&](auto wc) { t += xch[(decltype(wc)::value * NB + J) * 16 + c]; });  // same order in every wave
        y[J] = t;
      });
    }
  };
  // ---- right-hand side: column f of the last tile column, b[16 I + i] = T(I, NB - 1)[i][f - 16 (NB - 1)]
  float b[NB];
  {
    const int cf = f - 16 * (NB - 1);
    static_for<NB>([&](auto ic) {
      constexpr int I = decltype(ic)::value;
      constexpr int t = tile_of<NB>(I, NB - 1);
      b[I] = 0.f;
      if constexpr (t % NW == W) {
        float R[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) R[r] = bperm(4 * (16 * g + cf), T[t / NW][r]);  // lane (g, cf) over its row
        b[I] = to_col(R);
      }
    });
    combine(b);
    static_for<NB>([&](auto jc) { b[decltype(jc)::value] = live[decltype(jc)::value] ? b[decltype(jc)::value] : 0.f; });
  }
  // ---- y = A v.  Per tile 4 + 4 FMAs (direct half: rows of the tile against v_J; mirrored half: columns
  // against v_I in the row layout), per block row ONE transposed 4-register reduction and one ds_bpermute.
  const bool c1 = (c & 1) != 0, c2 = (c & 2) != 0;
  auto matvec = [&](const float (&v)[NB], float (&y)[NB]) {
    f32x2 ca[NB];
    static_for<NB>([&](auto jc) {
      ca[decltype(jc)::value] = f32x2{0.f, 0.f};
      y[decltype(jc)::value] = 0.f;
    });
    static_for<NB>([&](auto ic) {
      constexpr int I = decltype(ic)::value;
      if constexpr (cg_row_has_any<NB, NW, W, I>()) {
        f32x2 pr01 = {0.f, 0.f}, pr23 = {0.f, 0.f};
        if constexpr (cg_row_has_offdiag<NB, NW, W, I>()) {
          pr01 = f32x2{bperm(row_addr, v[I]), bperm(row_addr + 4, v[I])};
          pr23 = f32x2{bperm(row_addr + 8, v[I]), bperm(row_addr + 12, v[I])};
        }
        f32x2 ra01 = {0.f, 0.f}, ra23 = {0.f, 0.f};
        static_for<NB>([&](auto jc) {
          constexpr int J = decltype(jc)::value;
          if constexpr (J >= I && tile_of<NB>(I, J) % NW == W) {
            constexpr int s = tile_of<NB>(I, J) / NW;
            const f32x2 t01 = __builtin_shufflevector(T[s], T[s], 0, 1), t23 = __builtin_shufflevector(T[s], T[s], 2, 3);
            const f32x2 vj = {v[J], v[J]};
            ra01 = fma2(t01, vj, ra01);
            ra23 = fma2(t23, vj, ra23);
            if constexpr (J > I) ca[J] = fma2(t23, pr23, fma2(t01, pr01, ca[J]));
          }
        });
        y[I] = bperm(sel_addr, row16_sum4_transposed(ra01[0], ra01[1], ra23[0], ra23[1], c1, c2));
      }
    });
    static_for<NB>([&](auto jc) {
      constexpr int J = decltype(jc)::value;
      float t = ca[J][0] + ca[J][1];
      t += bperm(4 * (lane ^ 16), t);
      t += bperm(4 * (lane ^ 32), t);
      y[J] += t;
    });
    combine(y);
    static_for<NB>([&](auto jc) { y[decltype(jc)::value] = live[decltype(jc)::value] ? y[decltype(jc)::value] : 0.f; });
  };
  // vector operations on block pairs (see fma2: scalar FMAs); NB odd: the last block alone
  auto pair = [](const float (&u)[NB], int j) { return f32x2{u[j], u[j + 1]}; };
  auto dot = [&](const float (&u)[NB], const float (&v)[NB]) {
    f32x2 t2 = {0.f, 0.f};
    static_for<NB / 2>([&](auto jc) {
      constexpr int j = 2 * decltype(jc)::value;
      t2 = fma2(pair(u, j), pair(v, j), t2);
    });
    float t = t2[0] + t2[1];
    if constexpr (NB & 1) t = fmaf(u[NB - 1], v[NB - 1], t);
    return row16_sum(t);
  };
  // y = a * u + y
  auto axpy = [&](float a, const float (&u)[NB], float (&y)[NB]) {
    const f32x2 a2 = {a, a};
    static_for<NB / 2>([&](auto jc) {
      constexpr int j = 2 * decltype(jc)::value;
      const f32x2 t = fma2(a2, pair(u, j), pair(y, j));
      y[j] = t[0];
      y[j + 1] = t[1];
    });
    if constexpr (NB & 1) y[NB - 1] = fmaf(a, u[NB - 1], y[NB - 1]);
  };
  // ---- CG (cg.cu:36-231)
  float* xg = a.update + (size_t)row * f;
  float x[NB], r[NB], p[NB], ap[NB];
  static_for<NB>([&](auto jc) {
    constexpr int J = decltype(jc)::value;
    const float xv = xg[live[J] ? 16 * J + c : 0];  // warm start (cg.cu:48); dead lanes read element 0 and drop it
    x[J] = live[J] ? xv : 0.f;
  });
  matvec(x, ap);
  static_for<NB>([&](auto jc) {
    constexpr int J = decltype(jc)::value;
    r[J] = b[J] - ap[J];
    p[J] = r[J];
  });
  float rsold = dot(r, r);
#if CUMF_ABLATE
  int iters_run = 0;
#endif
  for (int iter = 0; iter < a.cg_iters; ++iter) {
#if CUMF_ABLATE
    ++iters_run;
#endif
    matvec(p, ap);
    const float pap = dot(p, ap);
    const float alpha = rsold / pap;
    axpy(alpha, p, x);
    axpy(-alpha, ap, r);
    const float rsnew = dot(r, r);
    if ((double)rsnew < 1e-4) break;  // CG_ERROR (cg.cu:31,195); uniform: every wave computes the same bits
    const float beta = rsnew / rsold;
    rsold = rsnew;
    // p = r + beta p
    const f32x2 b2 = {beta, beta};
    static_for<NB / 2>([&](auto jc) {
      constexpr int j = 2 * decltype(jc)::value;
      const f32x2 t = fma2(b2, pair(p, j), pair(r, j));
      p[j] = t[0];
      p[j + 1] = t[1];
    });
    if constexpr (NB & 1) p[NB - 1] = fmaf(beta, p[NB - 1], r[NB - 1]);
  }
  if (W == 0 && g == 0) {
    static_for<NB>([&](auto jc) {
      constexpr int J = decltype(jc)::value;
      if (live[J]) xg[16 * J + c] = x[J];
    });
  }
#if CUMF_ABLATE
  if ((a.dbg & 65536) && W == 0 && lane == 0) atomicAdd(&g_cg_hist[iters_run < 15 ? iters_run : 15], 1ull);
#endif
  {
    // fused train SSE: S - x.b - x.r - reg |x|^2 (see wave_tile_ff).  Every wave holds all the vectors (identical bits);
    // the one that owns the last diagonal tile -- entry (f, f) = sum r^2 -- reports.
    constexpr int NT1 = NB * (NB + 1) / 2;
    if constexpr ((NT1 - 1) % NW == W) {
      if (a.sse_bins != nullptr) {
        const float S = wave_tile_ff<NB>(T[(NT1 - 1) / NW], f) - reg;  // the diagonal carries reg in slot f too
        const float xb = dot(x, b), xr = dot(x, r), xx = dot(x, x);
        wave_sse_add(a.sse_bins, (double)S - (double)xb - (double)xr - (double)reg * (double)xx, rowlen, lane);
      }
    }
  }
}

// tiles of wave W from the dumped slots (summed in slot order), then the CG
template <int NB, int NW, int W>
__device__ __forceinline__ void cg_wave_body(float* smem, const KernelArgs& a, int row, int slot0, int nslots,
                                             int rowlen, int lane) {
  constexpr int NT = NB * (NB + 1) / 2;
  constexpr int TPW = (NT + NW - 1) / NW;
  f32x4 T[TPW];
#pragma unroll
  for (int s = 0; s < TPW; ++s) T[s] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int sl = 0; sl < nslots; ++sl) {
    const float* part = a.part + (size_t)(slot0 + sl) * NT * 256;
    static_for<TPW>([&](auto sc) {
      constexpr int t = W + NW * decltype(sc)::value;
      if constexpr (t < NT) {
#pragma unroll
        for (int r = 0; r < 4; ++r) T[decltype(sc)::value][r] += part[((size_t)t * 4 + r) * 64 + lane];
      }
    });
  }
  cg_wave_core<NB, NW, W>(T, smem, a, a.f, row, rowlen, lane);
}

}  // namespace cumf
