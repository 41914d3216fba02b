// als_route.cpp -- the route of a half-iteration: which kernels, Gram arithmetic and solvers a call of the fused update or
// the materialising pass runs on, decided once per call from the run-time switches and a few facts of the plan.  Host only:
// no HIP call, no allocation.
#include <cstdlib>

#include "als_internal.h"
#include "cumf_als_capi.h"

namespace cumf {

namespace {
int g_gram_mode = -1;      // -1: not read yet; kGram*
int g_presplit_mode = -2;  // -2: not read yet; CUMF_PRESPLIT_*
}  // namespace

void set_gram_mode(int mode) { g_gram_mode = (mode == kGramExact || mode == kGramFast) ? mode : kGramAuto; }
void set_presplit_mode(int mode) { g_presplit_mode = mode; }

Switches switches() {
  if (g_gram_mode < 0) {
    const char* e = getenv("CUMF_ALS_GRAM");  // exact | fast | split (default)
    g_gram_mode = (e && (e[0] == 'e' || e[0] == 'E')) ? kGramExact : (e && (e[0] == 'f' || e[0] == 'F')) ? kGramFast : kGramAuto;
  }
  if (g_presplit_mode == -2) {
    const char* e = getenv("CUMF_ALS_PRESPLIT");
    g_presplit_mode = (e && e[0] == '0') ? CUMF_PRESPLIT_OFF : (e && e[0] == '1') ? CUMF_PRESPLIT_ON
                      : (e && e[0] == '2') ? CUMF_PRESPLIT_VERIFY : CUMF_PRESPLIT_AUTO;
  }
  static const double presplit_mb = getenv("CUMF_ALS_PRESPLIT_MB") ? atof(getenv("CUMF_ALS_PRESPLIT_MB")) : 64.0;
  static const bool splitpk = !(getenv("CUMF_ALS_SPLITPK") && *getenv("CUMF_ALS_SPLITPK") == '0');
  static const bool short_cg = !getenv("CUMF_ALS_SHORT_CG") || atoi(getenv("CUMF_ALS_SHORT_CG")) != 0;
  const char* dual = getenv("CUMF_ALS_DUAL");
  const char* lu16 = getenv("CUMF_ALS_LU16");
  const char* lu_exact = getenv("CUMF_ALS_LU_EXACT");
  return Switches{g_gram_mode,
                  g_presplit_mode,
                  presplit_mb,
                  splitpk,
                  short_cg,
                  !dual || atoi(dual) != 0,
                  !lu16 || atoi(lu16) != 0,
                  !getenv("CUMF_ALS_NO_BATCHED"),
                  !getenv("CUMF_ALS_NO_WAVE_SOLVE"),
                  lu_exact && atoi(lu_exact) != 0};
}

// Round 6 (kArithPre, als_wave.hip): a gather table that lives in the caches -- the Netflix Theta side gathers X (7 MB), the
// hugewiki X side Theta (16 MB) -- is rewritten per call as bf16 h | m | l planes (1.5 x the bytes, the SAME bits the in-kernel
// split produces) and the Gram stage takes its MFMA operands from it with 16-byte LDS-DMA + transposing LDS reads instead of
// ~250 VALU instructions of split per 32 ratings.  An HBM-resident table (the Netflix X side gathers 192 MB of Theta) stays
// fp32: there the bytes are the roof.  CUMF_PRESPLIT_OFF never, _ON / _VERIFY whenever the shape allows, _AUTO: tables whose
// planes take at most presplit_mb MB, and every table from f = 144 on (presplit_pays_any_size).
static bool presplit_wanted(int f, long gather_rows, const Switches& sw) {
  if (sw.presplit == CUMF_PRESPLIT_OFF || sw.gram != kGramAuto || !presplit_supported(f) || gather_rows <= 0) return false;
  if (sw.presplit == CUMF_PRESPLIT_ON || sw.presplit == CUMF_PRESPLIT_VERIFY) return true;
  return presplit_pays_any_size(f) || (presplit_pays(f) && (double)gather_rows * presplit_pitch(f) <= sw.presplit_mb * 1048576.0);
}

// The one place that encodes the routing matrix:
//   path   f > 207: als_generic.hip (materialise only).  Gram mode exact: the workgroup kernels (CG f <= 128, LU f <= 207).
//          Otherwise NB = 1 (f <= 14; one tile, a 32-rating MFMA K and one wave per row are all overhead: 0.56 vs 3.4 ms per
//          iteration at f = 10) on the workgroup kernels, f = 16 .. 111 one wave per item, f = 112 .. 207 two waves per item
//          (CUMF_ALS_NO_BATCHED: the workgroup kernels).
//   arith  gram mode fast: the f16 words (fused LU / CG of the wave kernels); else the pre-split planes where presplit_wanted
//          (one wave: packed last block unless _VERIFY; two waves: kArithPre only); else the in-kernel split, with the
//          rating-only last block packed at f % 16 == 0 on one wave (not under _OFF / _VERIFY: the six-product forms that the
//          bit-identity tests compare).  Materialise: always the in-kernel split.
//   chunked rows  the wave CG (one wave per row up to f = 111, four above f = 128); f = 112 .. 128 stays on the 4-wave
//          solvers of als_reduce_kernel: 38.8 vs 56.3 ms (CG) per Netflix iteration at f = 128 -- one wave holding 45 tiles
//          spills and has nobody to overlap with.  LU and materialise: als_reduce_kernel.
//   whole rows  in the kernel that formed the Gram, except on two waves LU above NB = 9 and materialise: Gram -> dense slots of
//          the tile buffer -> als_reduce_kernel (two waves on a 200 x 200 elimination lose more than the round trip costs:
//          Netflix f = 200 112 vs 106 ms, f = 160 85 vs 78; f = 128 39.0 vs 41.6 the other way).
//   chunk first  one-wave LU plans with a FEW chunked rows (a Theta side with a handful of very long columns, < 25 % of the
//          ratings): their chunk items go first in a launch of their own, and the whole rows keep the instance without the
//          dump exit (no spilled accumulators).  When the chunks are most of the work (the Netflix X side:
//          86 % of the ratings) one combined launch stays: the whole rows fill the tail of the equal-sized chunk items
//          (profiles/r05/stage_variants_ab.txt).
//   short rows  CG plans on one wave, 32 <= f <= 128: the whole rows of at most kShortRow ratings never form their Gram.
//   dual rows  LU plans on one wave in the production pre-split form (kArithPrePk, f = 96 .. 111): the whole rows of
//          1 .. kDualMaxRow ratings (the plan lists them last in every item list) solve their n x n dual system
//          (als_dual.hip).  Rows without ratings stay (the reference's NaN).  CUMF_ALS_DUAL=0: none.
//   lu16   the one-wave LU of NB = 7 eliminates sixteen pivots per step (kLuPanel16, als_wave_lu.h); CUMF_ALS_LU16=0: the four-pivot
//          panels (the _p4 instances), which NB < 7 and the dual kernel keep (measured slower there: profiles/lu16/).
//   sse    every solver but two adds the train SSE of its rows: the workgroup CG of als_reduce_kernel, and its thread-grid LU
//          below NB = 7 -- the chunked rows of LU plans below f = 96 and of CG plans at f = 112 .. 128 are not covered.
Route route_for(int f, int mode, const PlanFacts& p, const Switches& sw) {
  Route r{};
  const int nb = nb_for_f(f);
  const bool wave_gram = sw.gram != kGramExact;
  if (f > kMaxF)
    r.path = mode == kModeMaterialize ? kPathGeneric : kPathNone;
  else if (wave_gram && nb >= 2 && nb <= kMaxWaveNB)
    r.path = kPathOneWave;
  else if (wave_gram && sw.batched && nb > kMaxWaveNB)
    r.path = kPathTwoWave;
  else
    r.path = (mode == kModeMaterialize || fused_supported(f, mode)) ? kPathWorkgroup : kPathNone;
  const bool one = r.path == kPathOneWave, wave = one || r.path == kPathTwoWave;

  r.arith = kArithSplit3;
  if (wave && mode != kModeMaterialize) {
    if (sw.gram == kGramFast) {
      r.table = kTableF16Words;
      r.arith = kArithFast;
    } else if (presplit_wanted(f, p.gather_rows, sw)) {
      r.table = kTablePlanes;
      r.arith = (one && sw.presplit != CUMF_PRESPLIT_VERIFY) ? kArithPrePk : kArithPre;
    } else if (one && sw.splitpk && (f & 15) == 0 && sw.presplit != CUMF_PRESPLIT_OFF &&
               sw.presplit != CUMF_PRESPLIT_VERIFY) {
      r.arith = kArithSplitPk;
    }
  }
  r.fc = (one && f == 100) ? 100 : 0;

  r.chunked = (wave && mode == kModeCG && sw.wave_solve && (one || f > kVecLd)) ? kSolveWaveCG : kSolveReduce;
  r.whole = (r.path == kPathTwoWave && mode != kModeCG && !(mode == kModeLU && nb <= kMaxFusedLuWaveNB)) ? kSolveTileBuffer
                                                                                                          : kSolveInKernel;
  r.chunk_first = one && mode == kModeLU && p.n_mrows > 0 && p.n_citems > 0 && p.n_witems > 0 && p.chunk_share < 0.25;
  r.n_short = (one && mode == kModeCG && sw.short_cg && short_cg_available(f)) ? p.n_short : 0;
  // the one-wave LU in the production pre-split form (never under CUMF_PRESPLIT_OFF / _VERIFY: those forms are compared bit
  // for bit); the row's own length decides, not what else the plan holds (the WHOLE and the combined launch agree bit for bit)
  const bool dual = one && mode == kModeLU && sw.dual && r.arith == kArithPrePk && nb == 7 && (f & 3) == 0 && f >= 96 &&
                    dual_rows_available(f);
  r.n_dual = dual ? p.n_dual : 0;
  r.n_dual_behind = r.n_dual > 0 ? p.n_empty : 0;
  r.lu16 = one && mode == kModeLU && sw.lu16 && lu16_default(nb);
  r.sse = wave && mode != kModeMaterialize &&
          (p.n_mrows == 0 || r.chunked == kSolveWaveCG || (mode == kModeLU && nb >= 7));
  return r;
}

}  // namespace cumf
