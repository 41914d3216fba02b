// als_internal.h -- the core declarations shared by the HIP kernels and the host side of libALS.so: constants, kernel
// arguments, routes, launchers, the plan and the scratch pool.  Implicit feedback, top-k, full ranking, NNLS and biased ALS
// each have a header of their own (als_implicit.h, als_topk.h, als_rank.h, als_nnls.h, als_bias.h) that only their own files
// include.
#ifndef CUMF_ALS_INTERNAL_H_
#define CUMF_ALS_INTERNAL_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <type_traits>

// Profiling build (make ablate -> libALS_ablate.so): the kernels additionally honour KernelArgs::dbg, switches that
// make the results WRONG on purpose (no solve, no Gram pass, ...) to time parts of a kernel.  The production
// library compiles none of it and exports no way to set it.
#ifndef CUMF_ABLATE
#define CUMF_ABLATE 0
#endif

namespace cumf {

constexpr int kThreads = 256;   // 4 waves of 64
constexpr int kStage = 32;      // gathered factor rows per LDS stage
constexpr int kVecLd = 128;     // pitch of the CG vectors in LDS (fused solve needs f <= 128)
constexpr int kMaxFusedNB = 9;  // f <= 128  ->  NB = f / 16 + 1 <= 9
constexpr int kMaxF = 207;      // NB <= 13: the range of the tile kernels (fused paths, MFMA Gram)
constexpr int kMaxFAny = 512;   // round 6: above kMaxF the reference's unfused data flow on two plain kernels (als_generic.hip)
constexpr int kMaxWaveNB = 7;   // wave-per-item kernels (als_wave.hip): f <= 111; register budget of one wave
// two-wave kernel: LU in place up to this NB (CG: always).  Round 5 measured 13 (f = 200 solved in place by the two Gram
// waves): Theta side 82.4 vs 74.4 ms through the tile buffer (profiles/r05/lu_rows_ab.txt)
constexpr int kMaxFusedLuWaveNB = 9;

enum { kModeCG = 0, kModeLU = 1, kModeMaterialize = 2, kModeLUExact = 3, kModeCGHalf = 4 };  // CGHalf: A stored as fp16

// Feature blocks of 16 including the slot that carries the rating value (RHS).
__host__ __device__ constexpr int nb_for_f(int f) { return f / 16 + 1; }
constexpr int kMaxNB = nb_for_f(kMaxF);  // 13
// LDS system matrix G: f rows, column f = RHS.  CG reads rows with 16-byte loads (pitch a
// multiple of 4 floats); the LU paths walk columns (odd pitch = conflict-free).
__host__ __device__ constexpr int solve_ldg(int f, int mode) { return mode == kModeCG ? ((f + 1 + 3) & ~3) : (f + 1); }
__host__ __device__ constexpr size_t solve_g_floats(int f, int mode) {
  return ((size_t)f * solve_ldg(f, mode) + 3) & ~(size_t)3;
}
// Register LU (fast path): packed upper-triangular row store (als_device.h: lu_row_off) + f
// pivot reciprocals.  f = 100: 29 520 B, below the 32 256 B of the stage buffers it aliases
// -> 5 workgroups per CU.
__host__ __device__ constexpr size_t lu_packed_floats(int nb) { return (size_t)256 * nb * (nb + 1) / 2 + 16 * nb; }
// + 2 x 16 multipliers of the panel owner + 16 zeros (accumulator LU)
__host__ __device__ constexpr size_t lu_lds_floats(int nb, int f) { return lu_packed_floats(nb) + (size_t)((f + 3) & ~3) + 48; }
constexpr int kCgExtraFloats = 12 * kVecLd;  // 4 per-wave operand copies + 2 x 4 partial mat-vecs
// whole LDS footprint of a solve on a full G: G + CG exchange buffers | G (exact-order LU)
__host__ __device__ constexpr size_t solve_lds_floats(int f, int mode) {
  return solve_g_floats(f, mode) + (mode == kModeCG ? (size_t)kCgExtraFloats : 0);
}

// Which (f, solver) pairs the fused Gram+solve kernel covers.
__host__ __device__ constexpr bool fused_supported(int f, int mode) {
  // CG keeps x, r, p, Ap as two registers per lane (elements lane and lane + 64): f <= 128 exactly, not
  // "NB <= 9" (f = 130..143 has NB = 9 too; found by tests/test_gpu_parity.py::test_doals_large_f)
  return mode == kModeLU ? nb_for_f(f) <= nb_for_f(kMaxF) : (f <= kVecLd && nb_for_f(f) <= kMaxFusedNB);
}

struct KernelArgs {
  // plan items (one workgroup each)
  const int* item_row;
  const long long* item_begin;
  const int* item_len;
  const int* item_slot;
  const int* item_rowlen;
  // chunked rows (reduce kernel)
  const int* mrow_row;
  const int* mrow_slot0;
  const int* mrow_nslots;
  const int* mrow_rowlen;
  float* part;
  // matrix + factors
  const int* colidx;
  const float* val;
  const float* gather;
  float* update;
  // materialise outputs
  float* tt;       // f x f Gram per row; holds _Float16 when tt_half (CUMF_TT_FP16 of als.cu:335-441)
  float* rhs;
  int tt_half;
  int tt_packed;   // tt receives the packed upper triangle, f (f + 1) / 2 floats per row (cumf_get_hermitian_packed)
  // dense_slots: item i (wave kernel) / row i (reduce kernel) of this launch uses slot i of `part` and
  // every item is dumped, none solved in place (batched "Gram -> tiles -> solver kernel" path)
  int dense_slots;
  int whole_only;  // host-only, no longer read (the route decides; the field keeps the kernels' argument layout)
  long long row_begin;
  int f;
  float lambda;
  int cg_iters;
  int dbg;  // ablation switches; read only by the kernels of the profiling build (-DCUMF_ABLATE=1, libALS_ablate.so)
  // gram mode "fast": `gather` points at the pre-split (h, l) f16 words of the factor table
  // (presplit_f16x2_kernel) and range violations are OR-ed into *fast_flag (bit 0: table, bit 1: ratings).
  // fast_words, pre_words, no_pack, whole_only: host-only and no longer read -- Route carries what they said; they stay
  // until a change of the kernels' argument layout removes them
  int fast_words;
  int* fast_flag;
  // round 6 (kArithPre): `gather` points at the pre-split bf16 h | m | l planes of the factor table (presplit_bf16x3_kernel),
  // rows of pre_pitch bytes
  int pre_words;
  unsigned pre_pitch;
  // fused train SSE (als.cu:979-991 folded into the Theta update): when not null, every whole-row item of a wave-kernel
  // launch adds sum_u (r_uv - x_u . theta_v)^2 of its row to sse_bins[item % kSseBins] (fp64 atomics)
  double* sse_bins;
  // the fp32 gather table itself (`gather` is replaced by the pre-split planes / f16 words of a launch that uses them): what
  // the Gram-free CG of short rows reads (als_short.hip)
  const float* gather_f32;
  int no_pack;
};
constexpr int kSseBins = 1024;

// Work lists of a plan as the launchers see them (device arrays of als_plan.cpp).
struct PlanLists {
  // all items, longest first (fused kernels)
  long n_items, n_mrows;
  // chunk items only (slot >= 0) and whole-row items only (slot < 0), each longest first
  long n_citems, n_witems;
  const int *c_row, *c_len, *c_slot, *c_rowlen;
  const long long* c_begin;
  const int *w_row, *w_len, *w_rowlen;
  const long long* w_begin;
  float* part2;      // dense-slot tile buffer of the batched path (lazily allocated), part2_rows slots
  long part2_rows;
  double chunk_share;  // share of the plan's ratings that sits in chunked rows
  long n_short;        // whole rows of at most kShortRow ratings: the LAST n_short items of the full list (and of the w list)
};
// Rows this short have a CG of their own that never forms the Gram matrix (als_short.hip); plans list them last.
constexpr int kShortRow = 32;
bool short_cg_available(int f);
hipError_t launch_short_cg(const KernelArgs& a, long n_items, hipStream_t stream);
// Whole rows of 1 .. kDualMaxRow ratings have an LU route of their own on the n x n dual system (als_dual.hip, five tile blocks;
// kDualMaxRow6: what a six-block instance would cover, counted by the plan, not built).  Plans list them behind every other
// item (longest first) and in front of the rows without ratings.
constexpr int kDualMaxRow = 79, kDualMaxRow6 = 95;
bool dual_rows_available(int f);
hipError_t launch_dual_rows(const KernelArgs& a, long n_items, hipStream_t stream);
hipError_t launch_solve_batched(const float* A, const float* b, float* x, long batch, int f, int mode, int cg_iters,
                                hipStream_t stream);
// Gram arithmetic of the fused / materialising passes.
//   kGramAuto:  fp32 values split exactly into three bf16 terms, six bf16 MFMA products per fp32
//               product, fp32 accumulation (als_wave.hip; fp32-class error, not bit-identical to a
//               fmaf chain); used where the wave kernels exist (all solvers and materialise, 16 <= f <= 207),
//   kGramExact: v_mfma_f32_16x16x4_f32, bit-identical to the reference thread's fmaf chain.
//   kGramFast (opt-in): the factor table pre-split into (h, l) f16 pairs of 4096 x, three f16 MFMA
//               products per fp32 product (22 significand bits); fused LU / CG passes of the wave
//               kernels only, everything else as kGramAuto; values must stay below 15.99 in magnitude.
enum { kGramAuto = 0, kGramExact = 1, kGramFast = 2 };
// Arithmetic of the wave kernels' Gram pass (als_wave.hip, where each form is described): the in-kernel bf16x3 split
// (kArithSplit3; kArithSplitPk with a rating-only last block packed), the pre-split f16 words of gram mode "fast"
// (kArithFast), the pre-split bf16 h | m | l planes (kArithPre; kArithPrePk with the last block packed).
enum { kArithSplit3 = 0, kArithFast = 1, kArithPre = 2, kArithPrePk = 3, kArithSplitPk = 4 };

// ---- Routing of a half-iteration (als_route.cpp): which kernels, arithmetic and solvers a call runs on.
// Every run-time knob that routes, read in one place.  gram / presplit: the environment (CUMF_ALS_GRAM,
// CUMF_ALS_PRESPLIT) on first use, then what cumf_set_gram_mode / cumf_set_presplit set; presplit_mb, splitpk,
// short_cg: the environment once per process; dual, lu16, batched, wave_solve, lu_exact: the environment on every call.
struct Switches {
  int gram;            // kGram*                       CUMF_ALS_GRAM = exact | fast | (split)
  int presplit;        // CUMF_PRESPLIT_*              CUMF_ALS_PRESPLIT = 0 | 1 | 2
  double presplit_mb;  // auto pre-split table cap     CUMF_ALS_PRESPLIT_MB (64)
  bool splitpk;        // kArithSplitPk wanted         CUMF_ALS_SPLITPK=0 turns it off
  bool short_cg;       // Gram-free CG of short rows   CUMF_ALS_SHORT_CG=0 turns it off
  bool dual;           // dual-form LU of short rows   CUMF_ALS_DUAL=0 turns it off
  bool lu16;           // 16-pivot steps, one-wave LU  CUMF_ALS_LU16=0: the four-pivot panels
  bool batched;        // two-wave path (f >= 112)     CUMF_ALS_NO_BATCHED turns it off
  bool wave_solve;     // wave CG of chunked rows      CUMF_ALS_NO_WAVE_SOLVE turns it off
  bool lu_exact;       // oracle-order batched LU      CUMF_ALS_LU_EXACT=1
};
Switches switches();
void set_gram_mode(int mode);
void set_presplit_mode(int mode);

// The facts of a plan the route depends on (all zero: the route of (f, mode) alone, e.g. cumf_fused_available).
struct PlanFacts {
  int nb;
  long n_mrows, n_citems, n_witems;
  double chunk_share;  // share of the plan's ratings that sits in chunked rows
  long n_short;        // whole rows of at most kShortRow ratings (the last items)
  long gather_rows;    // rows of the gather table (cumf_plan_set_gather_rows), 0: unknown
  long n_dual;         // whole rows of 1 .. kDualMaxRow ratings: the last items of the full and of the w list but for ...
  long n_empty;        // ... the whole rows without ratings, the very last
};
enum Path {
  kPathNone,       // no fused kernel for (f, solver)
  kPathGeneric,    // f > kMaxF, materialise only: the plain kernels of als_generic.hip
  kPathWorkgroup,  // als_item_kernel + als_reduce_kernel (f <= 14, gram mode exact)
  kPathOneWave,    // als_wave_kernel, one wave per item (16 <= f <= 111)
  kPathTwoWave,    // als_wave_multi_kernel, two waves per item, chunked rows and tiles batched apart (112 <= f <= 207)
};
enum Table { kTableNone, kTablePlanes, kTableF16Words };  // what the call prepares from the gather table
enum Solve {
  kSolveInKernel,    // by the wave(s) that formed the Gram
  kSolveTileBuffer,  // Gram dumped to the dense slots of the pooled tile buffer, then als_reduce_kernel
  kSolveReduce,      // als_reduce_kernel (the workgroup solvers) on the plan's slots
  kSolveWaveCG,      // als_wave_cg_kernel on the plan's slots
};
struct Route {
  Path path;
  int arith;         // kArith* of the wave kernels
  int fc;            // 100: the f = 100 instances of NB = 7 (the reference's get_hermitian100), else 0
  Table table;
  bool chunk_first;  // one-wave LU: the chunk items in a launch of their own, the whole rows on the instance without dumps
  long n_short;      // CG: the last n_short items go to the Gram-free CG (als_short.hip)
  Solve chunked;     // solver of the chunked rows
  Solve whole;       // solver of the whole rows
  bool sse;          // cumf_als_update_fused_sse covers every row
  // LU on one wave, pre-split table: the n_dual whole rows in front of the last n_dual_behind (rows without ratings: they
  // stay on the wave kernel) go to the dual-form kernel (als_dual.hip)
  long n_dual, n_dual_behind;
  bool lu16;  // one-wave LU: sixteen pivots per step (where lu16_default(NB)), else the four-pivot panels
};
// feature-block counts whose one-wave LU eliminates sixteen pivots per step by default: where it was measured faster
// (profiles/lu16/: NB = 7 Theta side 9.1 -> 8.7 ms; NB = 5 was 5.4 -> 5.7 ms at f = 64 -- one diagonal tile per three tiles of
// block row instead of one per four -- and keeps the four-pivot panels, as does the dual kernel's lu_wave_blocked<5>:
// 0.923 -> 0.934 ms)
constexpr bool lu16_default(int nb) { return nb == 7; }
Route route_for(int f, int mode, const PlanFacts& plan, const Switches& sw);
hipError_t launch_half_iteration(const KernelArgs& a, int mode, const Route& r, const PlanLists& lists, hipStream_t stream);

// unpack = 0: full (batch x f x f) -> packed (batch x f(f+1)/2); unpack = 1: `full` is the packed input,
// `packed` receives the mirrored full matrices
hipError_t launch_presplit(const float* src, unsigned* dst, size_t n, int* flag, hipStream_t stream);
// f > kMaxF (als_generic.hip): the fp32 f x f Gram batch + right-hand sides of the plan's items (whole rows), and the batched
// unpivoted LU in global memory (cumf_lu_solve_batched above f = 200): A is only read; the factors are formed in `work`,
// batch x f x f floats of the caller's (cublasSgetrfBatched overwrites A instead)
hipError_t launch_gram_generic(const KernelArgs& a, long n_items, hipStream_t stream);
hipError_t launch_lu_global(const float* A, float* work, const float* b, float* x, long batch, int f, hipStream_t stream);
// kArithPre: which (f, NB) have kernels on the pre-split bf16x3 table (als_wave.hip: CUMF_WAVE_PRE, presplit_shape_ok), the
// table's row pitch in bytes, and the kernel that writes it
// One-wave kernels (NB = 5, 7): strip of f % 16 in {0, 4} features; two-wave kernels (NB = 8 .. 13): f % 16 in {0, 4, 8}.
__host__ __device__ constexpr bool presplit_supported(int f) {
  return ((nb_for_f(f) == 7 || nb_for_f(f) == 5) && ((f & 15) == 0 || (f & 15) == 4)) ||
         (nb_for_f(f) > kMaxWaveNB && nb_for_f(f) <= nb_for_f(kMaxF) && (f & 3) == 0 && (f & 15) <= 8);
}
// ... and where CUMF_PRESPLIT_AUTO uses them: NB = 7 only.  At NB = 5 (f = 64) the 19 KB stage image costs the third wave per
// SIMD that the 160-register kernel otherwise gets (10 KB of dword chunks): measured SLOWER, Netflix f = 64 LU Theta side
// 5.6-5.9 -> 6.4-6.5 ms (profiles/r06/ab_presplit_f64_lu.txt); the kernels stay for CUMF_PRESPLIT_ON and the tests.
__host__ __device__ constexpr bool presplit_pays(int f) { return presplit_supported(f) && nb_for_f(f) >= 7; }
// ... and regardless of the table's size from NB = 10 on (f >= 144): there the two-wave kernel is bound by its matrix-pipe and
// split work, not by the gather -- Netflix f = 200, X side (a 384 MB table, 584 MB of planes): 28.8 -> 26.3 ms (CG), 29.5 ->
// 26.8 (LU); at f = 128 (NB = 9) the X side gains nothing (profiles/r06/ab_presplit_multi.txt)
__host__ __device__ constexpr bool presplit_pays_any_size(int f) { return presplit_supported(f) && nb_for_f(f) >= 10; }
__host__ __device__ constexpr unsigned presplit_pitch(int f) {
  return 96u * (f / 16) + ((f & 15) ? (nb_for_f(f) > kMaxWaveNB ? 64u : 32u) : 0u);
}
hipError_t launch_presplit3(const float* src, void* dst, long long rows, int f, hipStream_t stream);
hipError_t launch_pack_upper(const float* full, float* packed, long batch, int f, int unpack, hipStream_t stream);
void set_last_error(int code);  // read (and cleared) by cumf_last_error
// Timing pool, kernel names (als_launch.cpp)
void set_kernel_timing(bool on);
void note_item_kernel(const void* host_function);  // called by the launchers of the Gram(+solve) kernels
const void* last_item_kernel();
hipError_t last_kernel_ms(float* item_ms, float* reduce_ms);
// sums over every timed launch sequence since the previous call (or since timing was switched on), then resets
hipError_t kernel_ms_since_reset(float* item_ms, float* reduce_ms, int* launches);
// NB-independent kernels (als_common.hip)
hipError_t launch_quadratic_terms(const float* A, const float* b, const float* x, const float* reg, long batch, int f,
                                  double* out, hipStream_t stream);
hipError_t launch_sse(const float* val, const int* row, const int* col, const float* thetaT, const float* XT,
                      long count, int f, int surpass_nan, double* out, hipStream_t stream);
// CG with A streamed from global memory (f > 128); a_half: A stored as fp16
hipError_t launch_cg_global(const float* A, const float* b, float* x, long batch, int f, int cg_iters, bool a_half,
                            hipStream_t stream);

// ---- Per-NB entry points: function templates of the kernel files, each explicitly instantiated in the translation unit
// of its NB only (Makefile: als_kernels.hip once per CUMF_NB_SLICE, als_wave.hip once per CUMF_WAVE_NB and part).
// als_kernels.hip, NB = 1 .. kMaxNB; slice_solve also NB = 0: the oracle-order LU of CUMF_ALS_LU_EXACT.  slice_reduce_only: the
// solver of chunked rows (or of the dense slots of the tile buffer) on its own, behind the wave kernels' items
template <int NB>
hipError_t slice_half_iteration(const KernelArgs& a, int mode, long n_items, long n_mrows, hipStream_t stream);
template <int NB>
hipError_t slice_solve(const float* A, const float* b, float* x, long batch, int f, int mode, int cg_iters,
                       hipStream_t stream);
template <int NB>
hipError_t slice_reduce_only(const KernelArgs& a, int mode, const Route& r, long n_mrows, hipStream_t stream);
// als_wave.hip, NB = 2 .. kMaxNB; wave_lu_launch: NB <= kMaxWaveNB (part 1); wave_cg_hist: profiling build only
// whole: every item of the launch is a whole row (the LU instance without the dump exit)
template <int NB>
hipError_t wave_item_launch(const KernelArgs& a, int mode, const Route& r, bool whole, long n_items, hipStream_t stream);
template <int NB>
hipError_t wave_solve_launch(const KernelArgs& a, int mode, long n_rows, hipStream_t stream);
template <int NB>
hipError_t wave_lu_launch(const KernelArgs& a, const Route& r, bool whole, long n_items, hipStream_t stream);
template <int NB>
hipError_t wave_cg_hist(unsigned long long* out16);

// The one NB decoder: go(std::integral_constant<int, NB>{}) for LO <= nb <= HI, hipErrorInvalidValue otherwise.
template <int LO, int HI, class Go>
hipError_t with_nb(int nb, Go&& go) {
  if constexpr (LO > HI)
    return hipErrorInvalidValue;
  else
    return nb == LO ? go(std::integral_constant<int, LO>{}) : with_nb<LO + 1, HI>(nb, go);
}

// Declared here, shared by the host files, but not an exported symbol of the library.
#define CUMF_LOCAL __attribute__((visibility("hidden")))

// Scratch that outlives a call (als_scratch.cpp): process-wide, grow-only, one buffer per (device, stream, kind); an entry
// point that takes pooled scratch holds a ScratchLease until its last launch is enqueued (cumf_release_scratch waits for it).
enum {
  kScratchTiles = 0,
  kScratchWords = 1,
  kScratchPlanes = 2,
  // implicit feedback (als_implicit.cpp): Gram partials, per-chunk partial systems, materialised systems, right-hand sides,
  // compact solution vectors, fp64 Grams + loss partials
  kScratchImpGram = 3,
  kScratchImpSlots = 4,
  kScratchImpTT = 5,
  kScratchImpRhs = 6,
  kScratchImpX = 7,
  kScratchImpAux = 8,
  // top-k (als_topk.cpp): per-workgroup lists + survivor buffers, partial lists of the slabs, per-query metrics
  kScratchTopkWork = 9,
  kScratchTopkPart = 10,
  kScratchTopkMetrics = 11,
  // non-negative ALS (als_nnls.cpp): materialised systems, right-hand sides
  kScratchNnlsTT = 12,
  kScratchNnlsRhs = 13,
  // full ranking (als_rank.cpp): sorted held-out keys, buckets, valid thresholds per query, per-query metrics
  kScratchRankKeys = 14,
  kScratchRankHist = 15,
  kScratchRankValid = 16,
  kScratchRankMetrics = 17,
  // cumf_lu_solve_batched above f = 200: the batch the elimination in global memory factors in place of the caller's A
  kScratchLuWork = 18,
  // biased ALS (als_bias.cpp): the residual ratings of a half-iteration, fp64 partial sums of the SSE and the mean
  kScratchBiasResid = 19,
  kScratchBiasPart = 20,
  // matrix-free explicit CG (als_free.cpp): r | p, the segment partials of A v | b, r.r | done flags
  kScratchFreeVec = 21,
  kScratchFreePart = 22,
  kScratchFreeWords = 23,
};
int scratch_get(hipStream_t stream, int kind, size_t bytes, void** out);
// `count` elements of T (at least one) from the pool
template <typename T>
CUMF_LOCAL inline int scratch(hipStream_t stream, int kind, size_t count, T** out) {
  void* q = nullptr;
  const int rc = scratch_get(stream, kind, (count ? count : 1) * sizeof(T), &q);
  *out = static_cast<T*>(q);
  return rc;
}
// Bytes the pool holds for (current device, stream, kind) right now; 0: none
CUMF_LOCAL size_t scratch_capacity(hipStream_t stream, int kind);
// The current device's range flag of gram mode "fast" (one int, zeroed when first handed out)
CUMF_LOCAL int fast_flag_get(int** out);
struct ScratchLease {
  int dev = 0;
  ScratchLease();
  ~ScratchLease();
  ScratchLease(const ScratchLease&) = delete;
  ScratchLease& operator=(const ScratchLease&) = delete;
};
// Work lists of the implicit-feedback half-iterations, built on a plan at first use and freed with it (als_implicit.cpp).
struct ImplicitLists;
void free_implicit_lists(ImplicitLists* lists);
// The row segments of the matrix-free CGs, explicit and implicit, built on a plan at first use and freed with it (als_free.h,
// als_free.cpp).
struct FreeSegLists;
void free_seg_lists(FreeSegLists* lists);

}  // namespace cumf

// A half-iteration plan (cumf_plan_create, als_plan.cpp).
struct cumf_plan {
  long rows = 0, row_begin = 0, row_end = 0;
  int f = 0, nb = 0, chunk = 0;
  long long plan_nnz = 0;  // ratings of the planned rows
  long long entry_begin = 0;  // ... the first of them: entries [entry_begin, entry_begin + plan_nnz) of colidx / val
  long long chunk_nnz = 0;  // ... of which in chunked rows
  long n_items = 0, n_slots = 0, n_mrows = 0;
  long n_short = 0;  // whole rows of at most kShortRow ratings: the last n_short items (and the last of the w list)
  // whole rows of 1 .. kDualMaxRow / 1 .. kDualMaxRow6 ratings and without ratings: the item list and the w list end [.. | dual | empty]
  long n_dual = 0, n_dual6 = 0, n_empty = 0;
  int* d_item_row = nullptr;
  long long* d_item_begin = nullptr;
  int* d_item_len = nullptr;
  int* d_item_slot = nullptr;
  int* d_item_rowlen = nullptr;
  int* d_mrow_row = nullptr;
  int* d_mrow_slot0 = nullptr;
  int* d_mrow_nslots = nullptr;
  int* d_mrow_rowlen = nullptr;
  float* d_part = nullptr;
  char* d_block = nullptr;  // the device block all the index arrays below and above point into
  // chunk-only / whole-row-only item lists and the dense-slot tile buffer of the batched
  // "Gram -> tiles -> solver kernel" path (CG on the wave kernels' Gram)
  long n_citems = 0, n_witems = 0;
  int *d_c_row = nullptr, *d_c_len = nullptr, *d_c_slot = nullptr, *d_c_rowlen = nullptr;
  long long* d_c_begin = nullptr;
  int *d_w_row = nullptr, *d_w_len = nullptr, *d_w_rowlen = nullptr;
  long long* d_w_begin = nullptr;
  // gram mode "fast": rows of the gather table (cumf_plan_set_gather_rows)
  long gather_rows = 0;
  // implicit feedback: the long-row / empty-row lists of als_implicit.cpp (built on first use, freed with the plan)
  cumf::ImplicitLists* implicit = nullptr;
  // matrix-free CG, explicit and implicit: the row segments of als_free.cpp (built on first use, freed with the plan)
  cumf::FreeSegLists* free_seg = nullptr;
};

namespace cumf {

// What the entry points take from a plan (als_plan.cpp).  plan_lists: its work lists for launch_half_iteration; need_tiles:
// with the dense-slot tile buffer from the pool (Route::whole == kSolveTileBuffer).  plan_facts: what the route depends on.
CUMF_LOCAL int plan_lists(const cumf_plan* p, PlanLists* out, hipStream_t stream, bool need_tiles);
CUMF_LOCAL PlanFacts plan_facts(const cumf_plan* p);

// One launch: the dynamic-LDS opt-in above 64 KB, the launch, its error.  launch_item_kernel (NOTE): a Gram(+solve)
// kernel, also recorded for cumf_last_kernel_name.
template <bool NOTE = false, typename... P, typename... A>
hipError_t launch_kernel(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A&... args) {
  const void* fn = reinterpret_cast<const void*>(kernel);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  if (NOTE) note_item_kernel(fn);
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
  return hipGetLastError();
}
template <typename... P, typename... A>
hipError_t launch_item_kernel(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream,
                              const A&... args) {
  return launch_kernel<true>(kernel, grid, block, lds, stream, args...);
}

}  // namespace cumf

#define CUMF_HIP_CHECK(call)                                                                          \
  do {                                                                                                \
    hipError_t err__ = (call);                                                                        \
    if (err__ != hipSuccess) {                                                                        \
      fprintf(stderr, "HIP Error:\nFile = %s\nLine = %d\nReason = %s\n", __FILE__, __LINE__,          \
              hipGetErrorString(err__));                                                              \
      return (int)err__;                                                                              \
    }                                                                                                 \
  } while (0)

#endif  // CUMF_ALS_INTERNAL_H_
