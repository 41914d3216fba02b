// als_kernels.hip -- the workgroup kernels (256 threads = 4 wave roles per plan item or row) and their launchers.
//
// Which routes reach which kernel (route_for, als_route.cpp):
//   als_reduce_kernel  every route below f = 208: the chunked rows of a plan -- it sums their partial tiles in slot order
//                      and solves (LU: always; CG: f <= 14, f = 112 .. 128 and wherever the wave CG is switched off;
//                      materialise: always) -- and, on the two-wave route (f >= 112), the WHOLE rows of LU plans above
//                      NB = 9 and of materialise calls, out of the dense slots of the tile buffer (kSolveTileBuffer).
//                      The benchmark's LU half-iterations at f = 100 run it on the chunked rows of the X side.
//   solve_lds_kernel   no route: the standalone batched solvers of the C ABI (cumf_lu_solve_batched, the CG of
//                      materialised systems up to f = 128; NB = 0: the oracle-order LU of CUMF_ALS_LU_EXACT).
//   als_item_kernel    kPathWorkgroup only: gram mode exact (CUMF_ALS_GRAM=exact), f <= 14 (no wave kernel below
//                      NB = 2), and f >= 112 under CUMF_ALS_NO_BATCHED.  Not on the benchmark's path.
// The Gram pass of als_item_kernel is in als_wg_gram.h, the tile geometry and the accumulator hand-overs in
// als_wg_tiles.h, the in-LDS solvers in als_wg_solve.h; the LU on the accumulators is als_lu_wg.h, the register LU
// als_lu_reg.h.  Carrying out a route -- which launcher with which item lists -- is als_launch.cpp's job.
//
// The gram-mode-exact path (als_item_kernel + als_reduce_kernel) against the reference.  Per half-iteration the reference
// does (als.cu:727-964):
//   b   = R * Theta            cusparseScsrmm2 + cublasSgeam   (als.cu:750-757)
//   A_u = sum theta theta^T + lambda n_u I   get_hermitian100 / get_hermitianT10
//                                            (als.cu:443-569 / 575-659), one CUDA
//                                            block per row, 10x10 register tiles
//   x_u = A_u^-1 b_u           updateXWithCGKernel (cg.cu:36-231) or cuBLAS batched LU
// with the f x f Gram batch written to and re-read from device memory.
//
// What this path does instead (MI355X-first):
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
#include "als_wg_tiles.h"
#include "als_wg_gram.h"
#include "als_wg_solve.h"

namespace cumf {

// The file is compiled once per NB (Makefile: -DCUMF_NB_SLICE=1..13, the kernels of that feature-block count; 0: the
// oracle-order LU alone), so that the build runs in parallel.  Each object instantiates the entry points of its NB only
// (end of file).
#ifndef CUMF_NB_SLICE
#error "compile with -DCUMF_NB_SLICE=<feature blocks>"
#endif

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

// Geo<NB> deals the tiles to the four roles exactly as LuGeo<NB, 4> (als_lu_wg.h) wherever the LU runs on the accumulators:
// finish_row hands f32x4[Geo<NB>::TPW] to lu_solve_wg as LuAcc<NB, 4>.
template <int NB>
constexpr bool geo_is_lu_geo() {
  bool same = Geo<NB>::NT == LuGeo<NB, 4>::NT && Geo<NB>::TPW == LuGeo<NB, 4>::TPW;
  for (int w = 0; w < 4; ++w)
    for (int s = 0; s < Geo<NB>::TPW; ++s) same = same && Geo<NB>::tile(w, s) == LuGeo<NB, 4>::tile(w, s);
  return same;
}

// LU (default build): the whole solve runs on the accumulators inside the wave roles.
template <int NB, int MODE, int W, bool NEG>  // (declared, with NEG = false, in als_wg_gram.h for item_body)
__device__ __forceinline__ void finish_row(f32x4 (&acc)[Geo<NB>::TPW], float* smem, const KernelArgs& a, int row,
                                           int rowlen, int tid) {
  if constexpr (MODE == kModeLU && lu_on_accumulators(NB)) {
    static_assert(geo_is_lu_geo<NB>(), "Geo<NB> and LuGeo<NB, 4> disagree on the tiles of a wave role");
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

// Role of a wave: which tiles it owns (Geo::tile).  The LU on the accumulators loads the roles unevenly (role 0 runs the
// back substitution alone, the owner of a diagonal tile eliminates the pivot blocks, the last role's tiles stay live to
// the end) and the waves of a workgroup go to fixed SIMDs, so there the roles are rotated with the workgroup index:
// workgroups that share a CU differ in index / 256 (dispatch is round-robin over 8 XCDs x 32 CUs) and their heavy roles
// then sit on different SIMDs -- without the rotation one SIMD of every CU carries all the heavy roles.
template <int NB, int MODE>
__device__ __forceinline__ int wave_role(int tid, int index) {
  return (MODE == kModeLU && lu_on_accumulators(NB)) ? (((tid >> 6) + (index >> 8) + (index >> 10)) & 3) : (tid >> 6);
}

// ----------------------------------------------------------------------------------
// Kernel 1: one workgroup per plan item (item_body, als_wg_gram.h); a whole row is solved on the spot.
// ----------------------------------------------------------------------------------
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
  // the switch is written out here and in als_reduce_kernel: behind a helper that takes the body as a generic lambda the
  // kernels came out different (profiles/wg_split/README.md)
  switch (wave_role<NB, MODE>(tid, item)) {
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
#ifndef CUMF_REDUCE_LU_WGS
#define CUMF_REDUCE_LU_WGS 4
#endif
template <int NB, int MODE>
__global__ __launch_bounds__(kThreads, (NB >= 11 && MODE == kModeLU) ? CUMF_REDUCE_LU_WGS : 1) void als_reduce_kernel(const KernelArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int mr = blockIdx.x;
  const int row = a.mrow_row[mr];
  const int slot0 = a.dense_slots ? mr : a.mrow_slot0[mr];
  const int nslots = a.dense_slots ? 1 : a.mrow_nslots[mr];
  const int rowlen = a.mrow_rowlen[mr];
  switch (wave_role<NB, MODE>(tid, mr)) {
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

// ... with the widest gather the factor rows allow: 16-byte pieces when f % 4 == 0, else 8-byte (Stager)
template <int NB, int MODE>
static hipError_t launch_vt(const KernelArgs& a, long n_items, long n_mrows, hipStream_t stream) {
  return a.f % 4 == 0 ? launch_nb<NB, f32x4, MODE>(a, n_items, n_mrows, stream)
                      : launch_nb<NB, f32x2, MODE>(a, n_items, n_mrows, stream);
}

// the workgroup kernels: the items (als_item_kernel), then the chunked rows (als_reduce_kernel)
template <int NB>
hipError_t slice_half_iteration(const KernelArgs& a, int mode, long n_items, long n_mrows, hipStream_t stream) {
  if (mode == kModeMaterialize) return launch_vt<NB, kModeMaterialize>(a, n_items, n_mrows, stream);
  if constexpr (NB <= kMaxFusedNB) {
    if (mode == kModeCG && a.f <= kVecLd)  // cg_solve_lds holds two vector elements per lane: f <= 128
      return launch_vt<NB, kModeCG>(a, n_items, n_mrows, stream);
  }
  // the register LU keeps only the packed upper triangle in LDS: fused up to f = 200
  if (mode == kModeLU) return launch_vt<NB, kModeLU>(a, n_items, n_mrows, stream);
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

// The entry points of this translation unit's NB (Makefile: one object per CUMF_NB_SLICE).  Slice 0 is only the
// oracle-order LU (solve_lds_kernel<0, kModeLU>, CUMF_ALS_LU_EXACT); the NB-independent kernels are in als_common.hip.
#if CUMF_NB_SLICE == 0
template hipError_t slice_solve<0>(const float*, const float*, float*, long, int, int, int, hipStream_t);
#else
template hipError_t slice_half_iteration<CUMF_NB_SLICE>(const KernelArgs&, int, long, long, hipStream_t);
template hipError_t slice_solve<CUMF_NB_SLICE>(const float*, const float*, float*, long, int, int, int, hipStream_t);
template hipError_t slice_reduce_only<CUMF_NB_SLICE>(const KernelArgs&, int, const Route&, long, hipStream_t);
#endif

}  // namespace cumf
