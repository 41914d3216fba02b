// als_block.cpp -- the driver of a half-iteration of the iALS++ block solver (als_block.h): the arguments from the plan and its
// segment lists, the scratch, and the launches on the caller's stream.  Kernels: als_block.hip.
#include <hip/hip_runtime.h>

#include "als_block.h"

using namespace cumf;

int cumf::update_block(cumf_plan* p, const int* colidx, const float* val, const float* gather, const float* G, float* update,
                       float lambda, float alpha, int reg_mode, int sweeps, hipStream_t s) {
  const FreeSegLists* l = nullptr;
  int rc = plan_free_lists(p, &l);
  if (rc) return rc;
  const long rows = p->row_end - p->row_begin;
  if (rows <= 0) return 0;
  const int f = p->f, nb = (f + kBlockWidth - 1) / kBlockWidth;
  BlockArgs a{};
  a.seg_row = l->d_seg_row;
  a.seg_begin = l->d_seg_begin;
  a.seg_len = l->d_seg_len;
  a.row_seg0 = l->d_row_seg0;
  a.row_nseg = l->d_row_nseg;
  a.row_len = l->d_row_len;
  a.rows = rows;
  a.nseg = l->n_seg;
  a.ent0 = l->ent_begin;
  a.colidx = colidx;
  a.val = val;
  a.gather = gather;
  a.G = G;
  a.x = update + (size_t)p->row_begin * f;
  a.f = f;
  a.lambda = lambda;
  a.alpha = alpha;
  a.reg_mode = reg_mode;
  // the caller holds the ScratchLease
  if ((rc = scratch(s, kScratchBlockYhat, (size_t)(l->ent_end - l->ent_begin), &a.yhat)) ||
      (rc = scratch(s, kScratchBlockPart, (size_t)a.nseg * kBlockPart, &a.part)) ||
      (rc = scratch(s, kScratchBlockStep, (size_t)rows * kBlockWidth, &a.d)))
    return rc;
  CUMF_HIP_CHECK(launch_block_open(a, s));
  // yhat runs one block step behind x: the step of the very last block is never folded in, nothing reads it
  for (int sweep = 0; sweep < sweeps; ++sweep)
    for (int k = 0; k < nb; ++k) CUMF_HIP_CHECK(launch_block_step(a, k, sweep > 0 || k > 0, sweep == 0, s));
  return 0;
}
