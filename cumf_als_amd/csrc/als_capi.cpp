// als_capi.cpp -- the C ABI of the device-pointer entry points (include/cumf_als_capi.h) that is neither plan
// construction (als_plan.cpp) nor the scratch pool (als_scratch.cpp): the fused and materialising half-iterations, the
// batched solvers, pack / unpack, the SSE kernels, the gram / pre-split / timing switches, the error and kernel-name
// probes, and the C++ drop-in symbols of include/cg.h.  The profiling build (libALS_ablate.so) recompiles this file only.
#include <hip/hip_runtime.h>

#include <cxxabi.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "als_internal.h"
#include "cg.h"
#include "cumf_als_capi.h"

using namespace cumf;

namespace {

#if CUMF_ABLATE
// Ablation switches of the kernels, profiling build only (libALS_ablate.so; CUMF_ALS_DBG /
// cumf_set_debug_switches): any value but 0 makes the results wrong on purpose -- 1 = no solve, 2 = no Gram
// pass, 8 = every gather hits row 0, 16 = no gather DMA.
int g_debug_switches = -1;
int debug_switches() {
  if (g_debug_switches < 0) g_debug_switches = getenv("CUMF_ALS_DBG") ? atoi(getenv("CUMF_ALS_DBG")) : 0;
  return g_debug_switches;
}
#endif

KernelArgs base_args(const cumf_plan_t* p, const int* colidx, const float* val, const float* gather, int f,
                     float lambda) {
  KernelArgs a{};
  a.item_row = p->d_item_row;
  a.item_begin = p->d_item_begin;
  a.item_len = p->d_item_len;
  a.item_slot = p->d_item_slot;
  a.item_rowlen = p->d_item_rowlen;
  a.mrow_row = p->d_mrow_row;
  a.mrow_slot0 = p->d_mrow_slot0;
  a.mrow_nslots = p->d_mrow_nslots;
  a.mrow_rowlen = p->d_mrow_rowlen;
  a.part = p->d_part;
  a.colidx = colidx;
  a.val = val;
  a.gather = gather;
  a.gather_f32 = gather;
  a.row_begin = p->row_begin;
  a.f = f;
  a.lambda = lambda;
#if CUMF_ABLATE
  a.dbg = debug_switches();
#endif
  return a;
}

// Gram mode "fast": the factor table as (h, l) f16 words, rebuilt per call (the factors change every
// half-iteration: 2 x 192 MB of traffic for the Netflix X table, ~0.1 ms).
int fast_words(const cumf_plan_t* p, const float* gather, int f, hipStream_t stream, KernelArgs* a) {
  if (p->gather_rows <= 0) {
    fprintf(stderr, "cumf_als_update_fused: gram mode \"fast\" needs the row count of the gather table "
                    "(cumf_plan_set_gather_rows)\n");
    return (int)hipErrorInvalidValue;
  }
  const size_t n = (size_t)p->gather_rows * f;
  void* words = nullptr;
  int rc = scratch_get(stream, kScratchWords, n * sizeof(unsigned), &words);
  if (rc) return rc;
  int* flag = nullptr;
  rc = fast_flag_get(&flag);
  if (rc) return rc;
  CUMF_HIP_CHECK(launch_presplit(gather, static_cast<unsigned*>(words), n, flag, stream));
  a->gather = reinterpret_cast<const float*>(words);
  a->fast_flag = flag;
  return 0;
}

// Round 6 (kArithPre): the gather table as bf16 h | m | l planes, rebuilt per call (als_route.cpp: presplit_wanted).
int pre_words(const cumf_plan_t* p, const float* gather, int f, hipStream_t stream, KernelArgs* a) {
  void* planes = nullptr;
  const int rc = scratch_get(stream, kScratchPlanes, (size_t)p->gather_rows * presplit_pitch(f), &planes);
  if (rc) return rc;
  CUMF_HIP_CHECK(launch_presplit3(gather, planes, p->gather_rows, f, stream));
  a->gather = reinterpret_cast<const float*>(planes);
  a->pre_pitch = presplit_pitch(f);
  return 0;
}

thread_local int g_last_error = 0;  // per host thread: concurrent doALS calls do not see each other's state

}  // namespace


// Error state of the entry points that return a value instead of a code (cumf_doALS_ex returns NaN and sets
// this): 0 = none, otherwise a HIP error code or one of CUMF_ERR_*.  Reading clears it.
extern "C" int cumf_last_error(void) {
  const int e = g_last_error;
  g_last_error = 0;
  return e;
}
void cumf::set_last_error(int code) { g_last_error = code; }

// Demangled name of the Gram(+solve) kernel the last half-iteration of this process dispatched, as a profiler
// prints it (e.g. "cumf::als_wave_kernel<7, 1, 100, 0>"); empty before the first launch.
extern "C" int cumf_last_kernel_name(char* buf, int cap) {
  if (!buf || cap <= 0) return (int)hipErrorInvalidValue;
  buf[0] = 0;
  const void* fn = last_item_kernel();
  if (!fn) return 0;
  const char* mangled = hipKernelNameRefByPtr(fn, nullptr);
  if (!mangled) return 0;
  int status = 0;
  char* dem = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
  const char* name = (status == 0 && dem) ? dem : mangled;
  size_t len = strlen(name);
  // drop the parameter list -- the first '(' outside the template brackets ("float __vector(4)" is a template
  // argument of the workgroup kernels) -- and the "void " of a template instance
  int depth = 0;
  for (size_t i = 0; name[i]; ++i) {
    if (name[i] == '<') ++depth;
    if (name[i] == '>') --depth;
    if (name[i] == '(' && depth == 0) {
      len = i;
      break;
    }
  }
  if (strncmp(name, "void ", 5) == 0) {
    name += 5;
    len -= 5;
  }
  if (len >= (size_t)cap) len = (size_t)cap - 1;
  memcpy(buf, name, len);
  buf[len] = 0;
  free(dem);
  return 0;
}

// Can one fused call (RHS + Gram + solve) handle (f, solver)?  Even f with a route (route_for, als_route.cpp).
extern "C" int cumf_fused_available(int f, int solver) {
  const int mode = solver == CUMF_SOLVER_LU ? kModeLU : kModeCG;
  if (f <= 0 || (f % 2) != 0 || (solver != CUMF_SOLVER_CG && solver != CUMF_SOLVER_LU)) return 0;
  return route_for(f, mode, PlanFacts{}, switches()).path != kPathNone;
}

namespace {
int update_fused_impl(const cumf_plan_t* p, const int* colidx, const float* val, const float* gather, float* update, int f,
                      float lambda, int solver, int cg_iters, double* sse_bins, void* stream) {
  if (!p || f != p->f) {
    fprintf(stderr, "cumf_als_update_fused: plan/f mismatch\n");
    return (int)hipErrorInvalidValue;
  }
  if (!cumf_fused_available(f, solver)) {
    fprintf(stderr, "cumf_als_update_fused: f = %d with this solver needs the materialising path "
                    "(cumf_get_hermitian + cumf_*_solve_batched): the fused LU serves even f <= %d, the fused CG "
                    "too except in gram mode exact (the full system in LDS, f <= %d)\n", f, kMaxF, kVecLd);
    return (int)hipErrorInvalidValue;
  }
  ScratchLease lease;  // pooled tile buffer / pre-split table stay ours until the last launch below is enqueued
  KernelArgs a = base_args(p, colidx, val, gather, f, lambda);
  a.update = update;
  a.cg_iters = cg_iters;
  a.sse_bins = sse_bins;
  const int mode = (solver == CUMF_SOLVER_LU) ? kModeLU : kModeCG;
  const Route r = route_for(f, mode, plan_facts(p), switches());
  PlanLists lists{};
  int rc = plan_lists(p, &lists, static_cast<hipStream_t>(stream), r.whole == kSolveTileBuffer);
  if (!rc && r.table == kTableF16Words) rc = fast_words(p, gather, f, static_cast<hipStream_t>(stream), &a);
  if (!rc && r.table == kTablePlanes) rc = pre_words(p, gather, f, static_cast<hipStream_t>(stream), &a);
  if (rc) return rc;
  CUMF_HIP_CHECK(launch_half_iteration(a, mode, r, lists, static_cast<hipStream_t>(stream)));
  return 0;
}
}  // namespace

extern "C" int cumf_als_update_fused(const cumf_plan_t* p, const int* colidx, const float* val, const float* gather,
                                     float* update, int f, float lambda, int solver, int cg_iters, void* stream) {
  return update_fused_impl(p, colidx, val, gather, update, f, lambda, solver, cg_iters, nullptr, stream);
}

// Can the half-iteration of this plan also deliver the train SSE of its rows (cumf_als_update_fused_sse)?  Where every
// solver on its route adds it (Route::sse; route_for spells out the two gaps).
extern "C" int cumf_fused_sse_available(const cumf_plan_t* p, int solver) {
  if (!p || (solver != CUMF_SOLVER_CG && solver != CUMF_SOLVER_LU)) return 0;
  return route_for(p->f, solver == CUMF_SOLVER_LU ? kModeLU : kModeCG, plan_facts(p), switches()).sse;
}

// cumf_als_update_fused + the train SSE of the updated rows for free (als.cu:979-991 folded into the update, see
// wave_tile_ff in als_wave.hip): sum over the plan's rows of sum_u (r - x_u . t)^2 is ADDED, spread over the
// CUMF_SSE_BINS fp64 words of sse_bins (device memory, zeroed by the caller; the total is their sum).
extern "C" int cumf_als_update_fused_sse(const cumf_plan_t* p, const int* colidx, const float* val, const float* gather,
                                         float* update, int f, float lambda, int solver, int cg_iters, double* sse_bins,
                                         void* stream) {
  if (!sse_bins || !cumf_fused_sse_available(p, solver)) {
    fprintf(stderr, "cumf_als_update_fused_sse: not available for this plan (cumf_fused_sse_available)\n");
    return (int)hipErrorInvalidValue;
  }
  return update_fused_impl(p, colidx, val, gather, update, f, lambda, solver, cg_iters, sse_bins, stream);
}

namespace {
// storage: 0 = fp32 f x f (both triangles), 1 = fp16 f x f, 2 = fp32 packed upper triangle
int get_hermitian_any(const char* who, const cumf_plan_t* p, const int* colidx, const float* val, const float* gather,
                      void* tt, float* rhs, int f, float lambda, void* stream, int storage) {
  if (!p || f != p->f) {
    fprintf(stderr, "%s: plan/f mismatch\n", who);
    return (int)hipErrorInvalidValue;
  }
  ScratchLease lease;
  KernelArgs a = base_args(p, colidx, val, gather, f, lambda);
  a.tt = static_cast<float*>(tt);
  a.tt_half = storage == 1;
  a.tt_packed = storage == 2;
  a.rhs = rhs;
  const Route r = route_for(f, kModeMaterialize, plan_facts(p), switches());
  if (r.path == kPathGeneric) {  // above the tile kernels' range: the plain kernel of als_generic.hip, fp32 f x f storage only
    if (storage != 0) {
      fprintf(stderr, "%s: f = %d is above the tile kernels' range (%d): only the fp32 f x f batch (cumf_get_hermitian)\n", who, f, kMaxF);
      return (int)hipErrorInvalidValue;
    }
    CUMF_HIP_CHECK(launch_gram_generic(a, p->n_items, static_cast<hipStream_t>(stream)));
    return 0;
  }
  PlanLists lists{};
  const int rc = plan_lists(p, &lists, static_cast<hipStream_t>(stream), r.whole == kSolveTileBuffer);
  if (rc) return rc;
  CUMF_HIP_CHECK(launch_half_iteration(a, kModeMaterialize, r, lists, static_cast<hipStream_t>(stream)));
  return 0;
}
}  // namespace

extern "C" int cumf_get_hermitian(const cumf_plan_t* p, const int* colidx, const float* val, const float* gather,
                                  float* tt, float* rhs, int f, float lambda, void* stream) {
  return get_hermitian_any("cumf_get_hermitian", p, colidx, val, gather, tt, rhs, f, lambda, stream, 0);
}

extern "C" int cumf_get_hermitian_fp16(const cumf_plan_t* p, const int* colidx, const float* val, const float* gather,
                                       void* tt_half, float* rhs, int f, float lambda, void* stream) {
  return get_hermitian_any("cumf_get_hermitian_fp16", p, colidx, val, gather, tt_half, rhs, f, lambda, stream, 1);
}

// The Gram batch as packed upper triangles, written straight from the accumulators: what the multi-GPU
// Theta phase reduces across GPUs (hugewiki.cu:2703-2717 moves full f x f matrices) -- no f x f batch is
// materialised and no pack pass runs.
extern "C" int cumf_get_hermitian_packed(const cumf_plan_t* p, const int* colidx, const float* val,
                                         const float* gather, float* packed, float* rhs, int f, float lambda,
                                         void* stream) {
  return get_hermitian_any("cumf_get_hermitian_packed", p, colidx, val, gather, packed, rhs, f, lambda, stream, 2);
}

extern "C" int cumf_cg_solve_batched_fp16(const void* A_half, float* x, const float* b, long batch, int f,
                                          int cg_iters, void* stream) {
  if (f <= 0 || f > 256) return (int)hipErrorInvalidValue;
  CUMF_HIP_CHECK(launch_solve_batched(static_cast<const float*>(A_half), b, x, batch, f, kModeCGHalf, cg_iters,
                                      static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int cumf_cg_solve_batched(const float* A, float* x, const float* b, long batch, int f, int cg_iters,
                                     void* stream) {
  if (f <= 0 || f > kMaxFAny) return (int)hipErrorInvalidValue;  // above f = 128: cg_global_kernel, one thread per row of the system
  CUMF_HIP_CHECK(launch_solve_batched(A, b, x, batch, f, kModeCG, cg_iters, static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int cumf_lu_solve_batched(const float* A, const float* b, float* x, long batch, int f, void* stream) {
  if (f <= 0 || f > kMaxFAny) {
    fprintf(stderr, "cumf_lu_solve_batched: f = %d unsupported (f <= %d)\n", f, kMaxFAny);
    return (int)hipErrorInvalidValue;
  }
  if (f > 200) {
    // above the LDS-resident solvers: the elimination in global memory, in the operation order of the unpivoted Doolittle LU +
    // getrs (als_generic.hip).  cublasSgetrfBatched overwrites A with the factors (als.cu:77); here they are formed in a
    // pooled copy of the batch (batch x f x f floats), so that A stays intact as the header promises for every f.
    if (batch <= 0) return 0;
    ScratchLease lease;
    float* work = nullptr;
    const int rc = scratch(static_cast<hipStream_t>(stream), kScratchLuWork, (size_t)batch * f * f, &work);
    if (rc) return rc;
    CUMF_HIP_CHECK(launch_lu_global(A, work, b, x, batch, f, static_cast<hipStream_t>(stream)));
    return 0;
  }
  // CUMF_ALS_LU_EXACT=1: the LDS-resident elimination in the oracle's exact operation order
  // (bit-identical to oracle_lu); default: the register-resident symmetric elimination.
  const int mode = switches().lu_exact ? kModeLUExact : kModeLU;
  CUMF_HIP_CHECK(launch_solve_batched(A, b, x, batch, f, mode, 0, static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int cumf_pack_upper(const float* full, float* packed, long batch, int f, void* stream) {
  CUMF_HIP_CHECK(launch_pack_upper(full, packed, batch, f, 0, static_cast<hipStream_t>(stream)));
  return 0;
}
extern "C" int cumf_unpack_upper(const float* packed, float* full, long batch, int f, void* stream) {
  CUMF_HIP_CHECK(launch_pack_upper(packed, full, batch, f, 1, static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int cumf_sse(const float* val, const int* row, const int* col, const float* thetaT, const float* XT,
                        long count, int f, int surpass_nan, double* sse_out, void* stream) {
  // sse_kernel gathers the factor rows in 8-byte pairs: an odd f would misalign every other row and read one float past
  // the last one.  f = 0 is the sum of val^2 (doALS takes it once); the index arrays are still dereferenced then.
  const bool reads = count > 0;
  if (f < 0 || (f % 2) != 0 || count < 0 || !sse_out || (reads && (!val || !row || !col)) ||
      (reads && f > 0 && (!thetaT || !XT))) {
    fprintf(stderr, "cumf_sse: needs an even f >= 0 (got f = %d), count >= 0 (got %ld), sse_out, and for count > 0 val, row, "
                    "col and (f > 0) both tables\n", f, count);
    return (int)hipErrorInvalidValue;
  }
  CUMF_HIP_CHECK(launch_sse(val, row, col, thetaT, XT, count, f, surpass_nan, sse_out, static_cast<hipStream_t>(stream)));
  return 0;
}

// Train SSE from materialised systems: *sse_terms += sum over the batch of 2 x.b - x^T A x + reg[v] |x|^2 (fp64), so that
// sum_u (r - x_u . t)^2 over the batch's ratings = (their sum r^2) - that.  A: batch x f x f (symmetric, reg[v] = lambda n_v
// on the diagonal), b, x: batch x f, reg: batch floats; a system without ratings is marked by reg < 0 and skipped.
extern "C" int cumf_quadratic_sse_terms(const float* A, const float* b, const float* x, const float* reg, long batch, int f,
                                        double* sse_terms, void* stream) {
  if (!A || !b || !x || !reg || !sse_terms) return (int)hipErrorInvalidValue;
  CUMF_HIP_CHECK(launch_quadratic_terms(A, b, x, reg, batch, f, sse_terms, static_cast<hipStream_t>(stream)));
  return 0;
}

// The workgroup-per-item kernels (als_kernels.hip) address the gather table with 32-bit byte offsets
// (Stager::gather_pass); the wave-per-item kernels use 64-bit lane addresses.  Fail loudly instead of
// gathering garbage (VERDICT r01 / ADVICE r01: hugewiki X on one GPU is 20 GB).
extern "C" int cumf_check_gather_table(long gather_rows, int f, int solver, int materialize) {
  const int mode = materialize ? kModeMaterialize : (solver == CUMF_SOLVER_LU ? kModeLU : kModeCG);
  if (gather_rows < 0 || f <= 0) return (int)hipErrorInvalidValue;
  if (solver != CUMF_SOLVER_CG && solver != CUMF_SOLVER_LU) {
    fprintf(stderr, "cumf_als: solver %d is not an explicit-feedback solver (CUMF_SOLVER_CG or CUMF_SOLVER_LU)\n", solver);
    return (int)hipErrorInvalidValue;
  }
  if (f > kMaxF) return 0;  // als_generic.hip: 64-bit gather addresses
  const Path path = route_for(f, mode, PlanFacts{}, switches()).path;
  if (path == kPathOneWave || path == kPathTwoWave) return 0;  // the wave kernels: 64-bit addresses too
  const unsigned long long bytes = (unsigned long long)gather_rows * (unsigned long long)f * 4ull;
  if (bytes >= (1ull << 32)) {
    fprintf(stderr,
            "cumf_als: the gathered factor table is %llu bytes (%ld rows x f = %d); this solver / f combination "
            "runs the kernels with 32-bit gather offsets (limit 4 GiB).  Shard the gathered side (cumf_als_amd.dist) "
            "or use the LU solver with f <= %d (64-bit addressing).\n",
            bytes, gather_rows, f, 16 * kMaxWaveNB - 1);
    return (int)hipErrorInvalidValue;
  }
  return 0;
}

extern "C" int cumf_set_gram_mode(int mode) {
  if (mode != CUMF_GRAM_AUTO && mode != CUMF_GRAM_EXACT && mode != CUMF_GRAM_FAST) return (int)hipErrorInvalidValue;
  set_gram_mode(mode);
  return 0;
}
extern "C" int cumf_get_gram_mode(void) { return switches().gram; }

extern "C" int cumf_set_presplit(int mode) {
  if (mode != CUMF_PRESPLIT_AUTO && mode != CUMF_PRESPLIT_OFF && mode != CUMF_PRESPLIT_ON && mode != CUMF_PRESPLIT_VERIFY)
    return (int)hipErrorInvalidValue;
  set_presplit_mode(mode);
  return 0;
}
extern "C" int cumf_get_presplit(void) { return switches().presplit; }
extern "C" long cumf_presplit_pitch(int f) { return presplit_supported(f) ? (long)presplit_pitch(f) : 0; }
extern "C" int cumf_presplit_table(const float* table, void* planes, long rows, int f, void* stream) {
  if (!table || !planes || rows < 0 || !presplit_supported(f)) return (int)hipErrorInvalidValue;
  CUMF_HIP_CHECK(launch_presplit3(table, planes, rows, f, static_cast<hipStream_t>(stream)));
  return 0;
}

#if CUMF_ABLATE
// profiling build only (not declared in include/): see debug_switches() above
extern "C" int cumf_set_debug_switches(int switches) {
  if (switches < 0) return (int)hipErrorInvalidValue;
  g_debug_switches = switches;
  return 0;
}
// switch 65536: rows by the number of CG iterations they ran (bins 0 .. 15), read and cleared; f selects the kernels'
// feature-block count (the profiling build has NB = 5, 7, 13)
extern "C" int cumf_debug_cg_histogram(int f, unsigned long long* out16) {
  if (!out16) return (int)hipErrorInvalidValue;
  CUMF_HIP_CHECK(hipDeviceSynchronize());
  switch (nb_for_f(f)) {
    case 5: CUMF_HIP_CHECK(cumf::wave_cg_hist<5>(out16)); break;
    case 7: CUMF_HIP_CHECK(cumf::wave_cg_hist<7>(out16)); break;
    case 13: CUMF_HIP_CHECK(cumf::wave_cg_hist<13>(out16)); break;
    default: return (int)hipErrorInvalidValue;
  }
  return 0;
}
#endif

extern "C" int cumf_set_kernel_timing(int enable) {
  set_kernel_timing(enable != 0);
  return 0;
}

extern "C" int cumf_last_kernel_ms(float* item_kernel_ms, float* reduce_kernel_ms) {
  if (!item_kernel_ms || !reduce_kernel_ms) return (int)hipErrorInvalidValue;
  CUMF_HIP_CHECK(last_kernel_ms(item_kernel_ms, reduce_kernel_ms));
  return 0;
}

extern "C" int cumf_kernel_ms_since_reset(float* item_kernel_ms, float* reduce_kernel_ms, int* launches) {
  if (!item_kernel_ms || !reduce_kernel_ms || !launches) return (int)hipErrorInvalidValue;
  CUMF_HIP_CHECK(kernel_ms_since_reset(item_kernel_ms, reduce_kernel_ms, launches));
  return 0;
}

extern "C" void cumf_rand_init(float* a, long count, float scale, long seed) {
  if (seed >= 0) srand((unsigned)seed);
  for (long k = 0; k < count; ++k) a[k] = scale * ((float)rand() / (float)RAND_MAX);
}

extern "C" int cumf_als_version(void) { return 100; }
extern "C" const char* cumf_als_arch(void) { return "gfx950"; }

// cg.h:32, cg.cu:641-644: A holds halves (the reference casts the float* it is handed: `(half*)A`)
void updateXWithCGHost_tt_fp16(float* A, float* x, float* b, const int batchSize, const int f, const float cgIter) {
  int rc = cumf_cg_solve_batched_fp16(A, x, b, batchSize, f, (int)ceilf(cgIter), nullptr);
  hipError_t e = hipDeviceSynchronize();
  if (rc != 0 || e != hipSuccess) {
    fprintf(stderr, "updateXWithCGHost_tt_fp16 failed: %s\n", hipGetErrorString(rc ? (hipError_t)rc : e));
    exit(EXIT_FAILURE);
  }
}

// C++-linkage drop-in of the reference's inner solver API (cg.h:30, cg.cu:682-686):
// device pointers, synchronous, aborts on error like cudaCheckError (als.h:667-674).
void updateXWithCGHost(float* A, float* x, float* b, const int batchSize, const int f, const float cgIter) {
  int rc = cumf_cg_solve_batched(A, x, b, batchSize, f, (int)ceilf(cgIter), nullptr);
  hipError_t e = hipDeviceSynchronize();
  if (rc != 0 || e != hipSuccess) {
    fprintf(stderr, "updateXWithCGHost failed: %s\n", hipGetErrorString(rc ? (hipError_t)rc : e));
    exit(EXIT_FAILURE);
  }
}

// C++-linkage drop-in of the reference's fused Gram + CG host (cg.h:34-36, cg.cu:1190-1197; disabled at its only
// call site, als.cu:809-812: "performance not good").  DEVICE pointers, synchronous.  For the rows
// batch_offset .. m - 1 of the CSR matrix: A = sum theta theta^T + lambda * n_row * I over the row's columns
// (cg.cu:735-840), then cgIter warm-started CG steps on A x = ythetaT with x = XT (cg.cu:826-1186).  XT and
// ythetaT are BATCH-LOCAL: system b (row batch_offset + b) uses XT[b * F ...] and ythetaT[b * F ...].  (The
// reference kernel strides ythetaT by blockDim.x = 64 instead of F, cg.cu:941 -- a defect of the disabled
// code path that is not reproduced -- and hard-codes F = 100 in its loader; any f the library supports works
// here.)  The ratings themselves are not an argument (the right-hand side comes precomputed), so the Gram
// batch is formed with the materialising kernels, at most 4 GiB at a time, and handed to the batched CG.
void alsUpdateFeature100Host(const int batch_offset, const int* csrRowIndex, const int* csrColIndex,
                             const float lambda, const int m, const int F, const float* thetaT, float* XT,
                             float* ythetaT, int cgIter) {
  auto fail = [](const char* what, int code) {
    fprintf(stderr, "alsUpdateFeature100Host failed (%s): %s\n", what, hipGetErrorString((hipError_t)code));
    exit(EXIT_FAILURE);
  };
  if (batch_offset < 0 || m < 0 || !csrRowIndex || !csrColIndex || !thetaT || !XT || !ythetaT)
    fail("arguments", (int)hipErrorInvalidValue);
  const long rows = (long)m - batch_offset;
  if (rows <= 0) return;
  std::vector<int> rowptr((size_t)m + 1);
  hipError_t e = hipMemcpy(rowptr.data(), csrRowIndex, rowptr.size() * sizeof(int), hipMemcpyDeviceToHost);
  if (e != hipSuccess) fail("row pointer", (int)e);
  // 2^31 or more ratings: the 4-byte row pointer has wrapped (hugewiki.cu:1973 reads it as unsigned): widen it; a row
  // pointer that is not non-decreasing as unsigned values is rejected by the plan (negative row lengths)
  std::vector<long long> rowptr64((size_t)m + 1);
  {
    long long hi = 0;
    unsigned prev = (unsigned)rowptr[0];
    rowptr64[0] = prev;
    for (long i = 1; i <= m; ++i) {
      const unsigned cur = (unsigned)rowptr[(size_t)i];
      if (cur < prev) hi += 1ll << 32;
      rowptr64[(size_t)i] = hi + cur;
      prev = cur;
    }
  }
  // the rating slot of the gathered rows (the fused right-hand side) reads zeros: this entry point has no ratings
  // (val == nullptr: the kernels read their zero row instead)
  const size_t sys_bytes = (size_t)F * F * sizeof(float);
  const long per_batch = std::max<long>(1, (long)(((size_t)4 << 30) / sys_bytes));
  float* tt = nullptr;
  if ((e = hipMalloc(reinterpret_cast<void**>(&tt), (size_t)std::min(rows, per_batch) * sys_bytes)) != hipSuccess)
    fail("Gram batch", (int)e);
  for (long b0 = 0; b0 < rows; b0 += per_batch) {
    const long nb = std::min(per_batch, rows - b0);
    cumf_plan_t* plan = nullptr;
    int rc = cumf_plan_create(&plan, rowptr64.data(), 1, m, batch_offset + b0, batch_offset + b0 + nb, F, 0);
    if (rc) fail("plan", rc);
    rc = cumf_get_hermitian(plan, csrColIndex, nullptr, thetaT, tt, nullptr, F, lambda, nullptr);
    if (rc) fail("Gram", rc);
    rc = cumf_cg_solve_batched(tt, XT + (size_t)b0 * F, ythetaT + (size_t)b0 * F, nb, F, cgIter, nullptr);
    if (rc) fail("CG", rc);
    if ((e = hipDeviceSynchronize()) != hipSuccess) fail("kernels", (int)e);
    cumf_plan_destroy(plan);
  }
  (void)hipFree(tt);
}
