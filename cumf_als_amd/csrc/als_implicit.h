// als_implicit.h -- implicit feedback: what als_implicit.hip (compiled in two parts) / als_implicit_free.hip (kernels) and als_implicit.cpp (host side;
// include/cumf_implicit_capi.h) share.  als_nnls.cpp takes it too, for the empty-row helpers.
#ifndef CUMF_ALS_IMPLICIT_H_
#define CUMF_ALS_IMPLICIT_H_

#include "als_free.h"  // FreeArgs, which ImplicitFreeArgs extends
#include "als_internal.h"

namespace cumf {

constexpr int kImpGramSlab = 1024;    // table rows per workgroup of the Gram kernel (one fp32 partial each)
constexpr int kImpLossBlocks = 1024;  // workgroups of the loss pass (one fp64 partial each)
constexpr int kImpRegPlain = kFreeRegPlain;  // CUMF_IMPLICIT_REG_PLAIN (reg_u = lambda); else lambda n_u
struct ImplicitArgs {
  // items of the materialising kernel / the short-row CG (the plan's lists); item_dst: system index of an item's row
  // (nullptr: row - row_begin)
  const int* item_row;
  const long long* item_begin;
  const int* item_len;
  const int* item_slot;
  const int* item_rowlen;
  const int* item_dst;
  // rows cut into chunks (slot reduce); mrow_dst as item_dst
  const int* mrow_row;
  const int* mrow_slot0;
  const int* mrow_nslots;
  const int* mrow_rowlen;
  const int* mrow_dst;
  long long row_begin;
  const int* colidx;
  const float* val;
  const float* gather;
  const float* G;  // f x f Gram of `gather` (not read by the packed output mode)
  float* tt;       // systems, f x f each (packed output mode: upper triangles, f (f + 1) / 2 each)
  float* rhs;      // right-hand sides (may be null)
  float* slots;    // per-chunk partials, f x f + f each
  float* update;   // short-row CG: warm start in, solution out
  int f;
  float lambda, alpha;
  int reg_mode;
  int cg_iters;
};
size_t implicit_gram_part_floats(long rows, int f);
// G (fp32, may be null) and G64 (fp64, may be null) of a rows x f table; part: implicit_gram_part_floats floats
hipError_t launch_implicit_gram(const float* Y, long rows, int f, float* part, float* G, double* G64, hipStream_t stream);
// its last step: the slab partials summed in slab order (fp64) into both triangles of G and / or G64
hipError_t launch_implicit_gram_reduce(const float* part, long rows, int f, float* G, double* G64, hipStream_t stream);
// G = Y^T diag(row_w) Y, otherwise as launch_implicit_gram (at row_w = 1: its bits)
hipError_t launch_weighted_gram(const float* Y, const float* row_w, long rows, int f, float* part, float* G, double* G64,
                                hipStream_t stream);
// systems of items [0, n_items) of a's lists, then the n_mrows chunked rows
hipError_t launch_implicit_hermitian(const ImplicitArgs& a, long n_items, long n_mrows, hipStream_t stream);
// the same pass in the packed output mode: the partial systems of cumf_get_hermitian_implicit_partial -- a.tt is a batch of
// packed upper triangles (f (f + 1) / 2 floats each), a.G is not read
hipError_t launch_implicit_partial(const ImplicitArgs& a, long n_items, long n_mrows, hipStream_t stream);
// tt[b] = packed[b] (mirrored) + G, then + reg_add on the diagonal (cumf_implicit_finish)
hipError_t launch_implicit_finish(const float* packed, const float* G, float reg_add, float* tt, long batch, int f,
                                  hipStream_t stream);
// Gram-free CG of the whole rows of items [first, first + count) (at most kShortRow entries each)
hipError_t launch_implicit_short_cg(const ImplicitArgs& a, long first, long count, hipStream_t stream);
hipError_t launch_implicit_copy_rows(const int* rows, long count, int f, const float* in, float* out, bool scatter,
                                     hipStream_t stream);
hipError_t launch_implicit_zero_rows(const int* rows, long count, int f, float* x, hipStream_t stream);
// part: kImpLossBlocks doubles
hipError_t launch_implicit_loss(const int* rowptr, const int* colidx, const float* val, const float* XT, const float* thetaT,
                                long m, int f, float lambda, float alpha, int reg_mode, const double* Gx, const double* Gy,
                                double* part, double* out, hipStream_t stream);
// Table rows per workgroup (and fp32 partial) of the Gram: kImpGramSlab up to f = 128, more above, where a partial is f x f.
inline long implicit_gram_slab(int f) {
  const int FT = (f + 15) / 16;
  return FT <= 8 ? kImpGramSlab : (long)kImpGramSlab * ((FT + 7) / 8);
}
// The Gram partials of a table with 128 < f <= 512 (als_implicit_free.hip; launch_implicit_gram reduces them); row_w: nullptr,
// or the weight of each table row (launch_weighted_gram)
hipError_t launch_implicit_gram_wide(const float* Y, const float* row_w, long rows, int f, float* part, hipStream_t stream);
// The matrix-free CG (als_implicit_free.hip): the arguments and segments of als_free.h, plus G and the confidence weights.
struct ImplicitFreeArgs : FreeArgs {
  const float* G;  // f x f Gram of `gather`
  float alpha;
  int reg_mode;
};
// the passes of launch_free_pass, on the implicit kernels
hipError_t launch_implicit_free_pass(const ImplicitFreeArgs& a, int step, int cg_iters, hipStream_t stream);

// The plan's rows without stored entries (absolute row ids, device array) from the lists of als_implicit.cpp, built on
// first use.
int plan_empty_rows(cumf_plan* p, const int** rows, long* count);

}  // namespace cumf

#endif  // CUMF_ALS_IMPLICIT_H_
