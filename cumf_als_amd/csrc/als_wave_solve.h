// als_wave_solve.h -- what the wave kernels (als_wave.hip) do with a finished tile set: the tile epilogues, the CG on the
// accumulators, the fused train SSE.
//
//   * LU on the accumulators of the one wave (lu_wave_blocked): als_wave_lu.h, included here.
//   * CG on the accumulators (cg_wave_core): vectors in a column layout, the mat-vec on the upper tiles with DPP / ds_bpermute
//     reductions, 1, 2 or 4 waves per system.  (Its bperm stays a local lambda: als_device.h's changed its register assignment.)
#pragma once
#include "als_wave_gram.h"
#include "als_wave_lu.h"

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
