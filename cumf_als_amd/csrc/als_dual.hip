// als_dual.hip -- LU half-iteration of SHORT whole rows in their n x n DUAL form (f = 96 .. 111 on the pre-split table).
//
// A row of n ratings has A = T^T T + lambda n I with T its n x f block of gathered factor rows: rank n.  For n < f the
// wave kernel still factors the full (f + 1)-column system.  The same normal equations are solved by
//   x = T^T y,   (T T^T + lambda n I) y = r
// (push-through identity: T^T (T T^T + c I)^-1 = (T^T T + c I)^-1 T^T), and the n x n system K = T T^T has NBD = 5 tile
// blocks for n <= 79 -- 15 tiles instead of 28, the elimination lu_wave_blocked<5> (als_wave_lu.h, four-pivot panels) runs at f = 64 .. 79.  One wave per row:
//   operands  K's MFMA contracts over FEATURES, and a pre-split table row is [h: 96 bf16][m][l][strip] (als_wave_pre.h): the
//             eight K slots 8 g .. 8 g + 7 of lane (g, c) for feature chunk kc are 16 contiguous bytes of plane p of row
//             idx[16 I + c], at byte 192 p + 64 kc + 16 g -- ONE global_load_dwordx4 per (block I, plane, chunk) straight into
//             the operand registers.  No LDS image, no LDS-DMA, no transposing read; the same registers are the A operand of
//             block I and the B operand of block J.  Lanes of a row index >= n read the zero row.  One chunk in registers at a
//             time, three waves per SIMD (kDualWaves below).
//   products  the six of the Gram pass (lh, hl, mm, mh, hm, hh: small terms first) per tile and chunk, on the diagonal
//             tiles too (both triangles come out of the same products: nothing to symmetrise).  The strip (f % 16 == 4: four
//             features, 8 bytes per plane) is packed ALONG K instead: A = [h h h m m m l l], B = [h m l h m l h m] in the
//             eight 4-slot groups of one K = 32 MFMA -- eight of the nine plane products (ll dropped as in the Gram pass, ml
//             and lm kept) in ONE MFMA per tile.
//   system    the ratings go into column n' of the last block column, n' = max(n, 16 (NBD - 1)) the run-time size handed to
//             lu_wave_blocked<NBD, 0>; it adds reg = lambda n to every diagonal entry, so the padded rows n .. n' - 1 have
//             pivot lambda n, no coupling and a zero right-hand side.  y lands in this wave's LDS.
//   x         lane k holds x[k] and x[64 + k]: two FMAs per rating with row rho of the fp32 table, 40 rows in flight at once
//             (the accumulators are dead by then).
//   SSE       (K + lambda n I) y = r, so the residual r - T x = lambda n y: the row's train SSE is (lambda n)^2 sum y^2.
// Rounding differs from the primal route (another system is factored); parity is by the LU tolerance of the tests
// (tests/test_dual_rows_gpu.py).  The route (als_route.cpp) sends only whole rows of 1 .. 16 NBD - 1 ratings here.
#include <hip/hip_runtime.h>

#include "als_device.h"
#include "als_internal.h"
#include "als_lu_blocked.h"
#include "als_wave_gram.h"
#include "als_wave_lu.h"
#include "als_wave_solve.h"  // wave_sse_add

namespace cumf {

namespace {

constexpr int kDualFB = 6;                 // full feature blocks of the table row: f = 96 .. 111
constexpr int kDualPlane = 32 * kDualFB;   // bytes of one plane
constexpr int kDualChunks = kDualFB / 2;   // K = 32 feature chunks
constexpr int kDualStrip = 96 * kDualFB;   // byte offset of the strip
// Three waves per SIMD (<= 168 registers: 60 accumulators + ONE chunk of 60 operand registers): the other waves cover the
// loads, and their VALU-bound eliminations run beside this wave's bf16 MFMAs.  Measured against two waves with a chunk of
// operands prefetched in registers (214 registers): Netflix Theta side 8.98 .. 9.16 vs 9.16 .. 9.30 ms
// (profiles/dual_rows/variants_time_halves.txt).
constexpr int kDualWaves = 3;
constexpr int kDualPass = 40;  // fp32 rows in flight in the back projection (80 registers)

// a generic pointer known to point to global memory, as one the compiler loads through with global_load (not flat_load)
template <class T>
__device__ __forceinline__ __attribute__((address_space(1))) const T* as_global(const void* p) {
  return reinterpret_cast<__attribute__((address_space(1))) const T*>(reinterpret_cast<unsigned long long>(p));
}

template <int NBD>
__host__ __device__ constexpr int dual_lds_floats() {
  return wave_lu_lds_floats<NBD>(16 * NBD - 1) + 16 * NBD + 16;  // the LU's buffers, then y
}

// feature chunk KC of every block's three planes, straight into the operand layout; ptr[I]: table row of rating 16 I + c
// + 16 g
template <int NBD, int KC>
__device__ __forceinline__ void dual_load_chunk(const char* const (&ptr)[NBD], u32x4 (&op)[NBD][3]) {
  static_for<NBD>([&](auto ic) {
    constexpr int I = decltype(ic)::value;
    static_for<3>([&](auto pc) {
      constexpr int p = decltype(pc)::value;
      op[I][p] = *as_global<u32x4>(ptr[I] + kDualPlane * p + 64 * KC);
    });
  });
}
// the six plane products of one chunk on every tile
template <int NBD>
__device__ __forceinline__ void dual_products(const u32x4 (&op)[NBD][3], f32x4 (&acc)[NBD * (NBD + 1) / 2]) {
  static_for<6>([&](auto prc) {
    constexpr int PROD = decltype(prc)::value;  // lh, hl, mm, mh, hm, hh
    constexpr int pa = PROD == 0 ? 2 : (PROD == 2 || PROD == 3) ? 1 : 0;
    constexpr int pb = PROD == 1 ? 2 : (PROD == 2 || PROD == 4) ? 1 : 0;
    static_for<NBD*(NBD + 1) / 2>([&](auto tc) {  // consecutive MFMAs hit different accumulators
      constexpr int t = decltype(tc)::value;
      constexpr int I = tile_I<NBD>(t), J = tile_J<NBD>(t);
      acc[t] = mfma_bf16(op[I][pa], op[J][pb], acc[t]);
    });
  });
}

template <int NBD>
__global__ __launch_bounds__(64, kDualWaves) void als_dual_kernel(const KernelArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NT = NBD * (NBD + 1) / 2;
  constexpr int kMaxN = 16 * NBD - 1;
  const int lane = threadIdx.x;
  const int item = blockIdx.x;
  const int row = a.item_row[item];
  const long long begin = a.item_begin[item];
  const int n = a.item_len[item];  // the whole row, 1 <= n <= kMaxN (the route's condition)
  const int f = a.f;
  const int c = lane & 15, g = lane >> 4;
  auto bperm_i = [](int addr, int v) { return __builtin_amdgcn_ds_bpermute(addr, v); };

  // rating rho = lane and 64 + lane of the row: column index and value
  const bool l0 = lane < n, l1 = 64 + lane < n;
  const int i0 = l0 ? a.colidx[begin + lane] : 0, i1 = l1 ? a.colidx[begin + 64 + lane] : 0;
  const float r0 = (l0 && a.val != nullptr) ? a.val[begin + lane] : 0.f;
  const float r1 = (l1 && a.val != nullptr) ? a.val[begin + 64 + lane] : 0.f;

  // table row of rating 16 I + c, + this lane group's 16 bytes of a chunk
  const char* ptr[NBD];
  static_for<NBD>([&](auto ic) {
    constexpr int I = decltype(ic)::value;
    const int idx = bperm_i(4 * ((16 * I + c) & 63), 16 * I < 64 ? i0 : i1);
    const char* p = reinterpret_cast<const char*>(a.gather) + (unsigned long long)(unsigned)idx * a.pre_pitch;
    ptr[I] = (16 * I + c < n ? p : reinterpret_cast<const char*>(g_wave_zeros)) + 16 * g;
  });

  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- K = T T^T
  static_for<kDualChunks>([&](auto kcc) {
    u32x4 op[NBD][3];  // [block][plane h, m, l]
    dual_load_chunk<NBD, decltype(kcc)::value>(ptr, op);
    dual_products<NBD>(op, acc);
  });
  if ((f & 15) != 0) {  // wave-uniform: the strip, packed along K
    const bool g0 = g == 0, g1 = g == 1, g2 = g == 2, g03 = g == 0 || g == 3;
    u32x4 A[NBD], B[NBD];
    static_for<NBD>([&](auto ic) {
      constexpr int I = decltype(ic)::value;
      const char* sp = ptr[I] + (kDualStrip - 16 * g);
      const u32x2 h = *as_global<u32x2>(sp), m = *as_global<u32x2>(sp + 8), l = *as_global<u32x2>(sp + 16);
      const u32x2 alo = (g0 || g1) ? h : (g2 ? m : l), ahi = g0 ? h : ((g1 || g2) ? m : l);
      const u32x2 blo = g03 ? h : (g1 ? l : m), bhi = g03 ? m : (g1 ? h : l);
      A[I] = u32x4{alo[0], alo[1], ahi[0], ahi[1]};
      B[I] = u32x4{blo[0], blo[1], bhi[0], bhi[1]};
    });
    static_for<NT>([&](auto tc) {
      constexpr int t = decltype(tc)::value;
      constexpr int I = tile_I<NBD>(t), J = tile_J<NBD>(t);
      acc[t] = mfma_bf16(A[I], B[J], acc[t]);
    });
  }

  // ---- the ratings as column n' of the last block column (row n' >= n of K is zero: the column held zeros)
  const int np = n > 16 * (NBD - 1) ? n : 16 * (NBD - 1);
  const int cr = np - 16 * (NBD - 1);
  static_for<NBD>([&](auto ic) {
    constexpr int I = decltype(ic)::value;
    constexpr int t = tile_of<NBD>(I, NBD - 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rho = 16 * I + 4 * g + r;
      const float v = __builtin_bit_cast(float, bperm_i(4 * (rho & 63), __builtin_bit_cast(int, 16 * I < 64 ? r0 : r1)));
      acc[t][r] = c == cr ? v : acc[t][r];
    }
  });

  // ---- (K + lambda n I) y = r
  const float reg = (float)n * a.lambda;
  float* ybuf = smem + wave_lu_lds_floats<NBD>(kMaxN);
  if (lane < 32) ybuf[16 * (NBD - 1) + lane] = 0.f;  // y past n' reads as zero below (the LU writes y[0 .. n') behind this)
  const float ssq = lu_wave_blocked<NBD, 0, kLuPanel4>(acc, smem, np, reg, ybuf, lane);
  __syncthreads();  // one wave: orders the writes of y before the reads below
  if (a.sse_bins != nullptr) {
    const float yy = wave_sum_uniform(ssq);
    wave_sse_add(a.sse_bins, (double)reg * (double)reg * (double)yy, n, lane);
  }

  // ---- x = T^T y on the fp32 table: kDualPass rows in flight, then two FMAs per rating (rho >= n: the row of the item's last
  // rating, in bounds, times y = 0).  Lanes whose second feature is past f re-read their first and drop the sum.
  const int off1 = 64 + lane < f ? 64 + lane : lane;
  float x0 = 0.f, x1 = 0.f;
  static_for<(kMaxN + kDualPass) / kDualPass>([&](auto pc) {
    constexpr int r0p = kDualPass * decltype(pc)::value;
    if (r0p < n) {  // uniform
      float T0[kDualPass], T1[kDualPass];
      static_for<kDualPass / 8>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        if (r0p + 8 * q < n) {  // uniform
          static_for<8>([&](auto ec) {
            constexpr int e = 8 * q + decltype(ec)::value, rho = r0p + e;
            const int rc = rho < n ? rho : n - 1;
            const int idx = __builtin_amdgcn_readlane(rho < 64 ? i0 : i1, rc & 63);
            const auto base = as_global<float>(a.gather_f32 + (size_t)(unsigned)idx * f);
            T0[e] = base[lane];
            T1[e] = base[off1];
          });
        }
      });
      static_for<kDualPass / 8>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        if (r0p + 8 * q < n) {  // uniform
          static_for<8>([&](auto ec) {
            constexpr int e = 8 * q + decltype(ec)::value, rho = r0p + e;
            const float y = ybuf[rho];
            x0 = fmaf(T0[e], y, x0);
            x1 = fmaf(T1[e], y, x1);
          });
        }
      });
    }
  });
  const bool f0 = lane < f, f1 = 64 + lane < f;
  float* xg = a.update + (size_t)row * f;
  if (f0) xg[lane] = x0;
  if (f1) xg[64 + lane] = x1;
}

}  // namespace

// the shapes with a dual kernel: the pre-split table rows of six full feature blocks (+ the four-feature strip)
bool dual_rows_available(int f) { return nb_for_f(f) == 7 && presplit_supported(f); }

// items [0, n_items) of the lists in `a` (the caller has advanced the list pointers to the plan's rows of 1 .. kDualMaxRow
// ratings); a.gather: the pre-split planes, a.gather_f32: the fp32 table
hipError_t launch_dual_rows(const KernelArgs& a, long n_items, hipStream_t stream) {
  if (n_items <= 0) return hipSuccess;
  if (!dual_rows_available(a.f) || a.gather_f32 == nullptr || a.pre_pitch != presplit_pitch(a.f)) return hipErrorInvalidValue;
  static_assert(kDualMaxRow == 16 * 5 - 1, "NBD = 5");
  return launch_kernel(als_dual_kernel<5>, dim3((unsigned)n_items), dim3(64), dual_lds_floats<5>() * sizeof(float), stream, a);
}

}  // namespace cumf
