// als_wg_tiles.h -- the accumulator tiles of the workgroup kernels (als_kernels.hip): which of the four wave roles of a
// workgroup holds which 16 x 16 tile of the upper triangle of [A | b] (Geo, for_each_tile), and where a role's tiles go
// after the Gram pass -- LDS for the in-LDS solvers, global memory for the materialised Gram, the partial-tile scratch of
// chunked rows and back.
#ifndef CUMF_ALS_WG_TILES_H_
#define CUMF_ALS_WG_TILES_H_

#include <hip/hip_runtime.h>

#include <type_traits>

#include "als_device.h"
#include "als_internal.h"

namespace cumf {

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

// The tiles of wave role W: body(slot, tile), both as std::integral_constant, for every accumulator slot that holds a tile.
template <int NB, int W, typename F>
__device__ __forceinline__ void for_each_tile(F&& body) {
  static_for<Geo<NB>::TPW>([&](auto sc) {
    constexpr int t = Geo<NB>::tile(W, decltype(sc)::value);
    if constexpr (t < Geo<NB>::NT) body(sc, std::integral_constant<int, t>{});
  });
}

// Accumulator tiles -> LDS, tile-major ([tile][16][16], rows permuted by tiled_row): the
// hand-over to lu_solve_reg, whose threads pick their elements up with TileLoad.
template <int NB, int W>
__device__ __forceinline__ void tiles_to_tiled(const f32x4 (&acc)[Geo<NB>::TPW], float* __restrict__ T,
                                               float reg, int lane) {
  const int c = lane & 15, kk = lane >> 4;
  for_each_tile<NB, W>([&](auto sc, auto tc) {
    constexpr int s = decltype(sc)::value, t = decltype(tc)::value;
    constexpr int I = tile_I<NB>(t), J = tile_J<NB>(t);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = acc[s][r];
      if (I == J && 4 * kk + r == c) v += reg;  // lambda * n_u on the diagonal (als.cu:545-557)
      T[256 * t + (4 * r + kk) * 16 + c] = v;
    }
  });
}

// Accumulator tile -> LDS system matrix G (f x ldg, column f = RHS).  C/D layout of
// the 16x16 MFMA: lane l, register r holds D[4*(l>>4) + r][l & 15].
template <int NB, int W>
__device__ __forceinline__ void tiles_to_lds(const f32x4 (&acc)[Geo<NB>::TPW], float* __restrict__ G,
                                             int ldg, int f, float reg, int lane) {
  const int c = lane & 15, kk = lane >> 4;
  for_each_tile<NB, W>([&](auto sc, auto tc) {
    constexpr int s = decltype(sc)::value, t = decltype(tc)::value;
    constexpr int I = tile_I<NB>(t), J = tile_J<NB>(t);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * I + 4 * kk + r, j = 16 * J + c;
      float v = acc[s][r];
      if (I == J && i == j) v += reg;                    // lambda * n_u on the diagonal (als.cu:545-557)
      if (i < f && j <= f) G[i * ldg + j] = v;           // j == f: b_i = sum r * theta[i]
      if (I != J && i < f && j < f) G[j * ldg + i] = v;  // mirror
    }
  });
}

// Accumulator tile -> row-major f x f Gram in global memory (both triangles,
// lambda * n on the diagonal: als.cu:545-566) + RHS.
template <int NB, int W, typename T>
__device__ __forceinline__ void tiles_to_global(const f32x4 (&acc)[Geo<NB>::TPW], T* __restrict__ tt,
                                                float* __restrict__ rhs, int f, float reg, int lane,
                                                bool packed = false) {
  const int c = lane & 15, kk = lane >> 4;
  for_each_tile<NB, W>([&](auto sc, auto tc) {
    constexpr int s = decltype(sc)::value, t = decltype(tc)::value;
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
  });
}

// Partial tiles <-> global scratch, in accumulator layout ([slot][tile][reg][lane]:
// every store/load is one coalesced 256-byte wave access).
template <int NB, int W>
__device__ __forceinline__ void tiles_to_partial(const f32x4 (&acc)[Geo<NB>::TPW], float* __restrict__ part,
                                                 int lane) {
  for_each_tile<NB, W>([&](auto sc, auto tc) {
    constexpr int s = decltype(sc)::value, t = decltype(tc)::value;
#pragma unroll
    for (int r = 0; r < 4; ++r) part[((size_t)t * 4 + r) * 64 + lane] = acc[s][r];
  });
}
// NEG: the sum of the partial tiles NEGATED (what the blocked workgroup LU eliminates: lu_solve_blocked_wg)
template <int NB, int W, bool NEG = false>
__device__ __forceinline__ void partial_accumulate(f32x4 (&acc)[Geo<NB>::TPW], const float* __restrict__ part,
                                                   int lane) {
  for_each_tile<NB, W>([&](auto sc, auto tc) {
    constexpr int s = decltype(sc)::value, t = decltype(tc)::value;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = part[((size_t)t * 4 + r) * 64 + lane];
      acc[s][r] = NEG ? acc[s][r] - v : acc[s][r] + v;
    }
  });
}

}  // namespace cumf

#endif  // CUMF_ALS_WG_TILES_H_
