// als_implicit.cpp -- host side of implicit-feedback ALS (include/cumf_implicit_capi.h): the route of a half-iteration,
// the long-row lists it needs on a plan, and the C ABI.  Kernels: als_implicit.hip.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <unordered_map>
#include <vector>

#include "als_implicit.h"
#include "cumf_als_capi.h"
#include "cumf_implicit_capi.h"

using namespace cumf;

namespace cumf {

// Lists of a plan that only the implicit half-iterations read, built on first use (the plan's own lists stay as they are).
// The plan lists its whole rows of at most kShortRow entries as the LAST n_short items; the items before them -- every chunk
// and every longer whole row -- are the "long" items whose systems the CG route materialises into a compact batch.
struct ImplicitLists {
  long n_long_items = 0;  // items [0, n_long_items) of the plan's list
  long n_long = 0;        // their rows, in the order of first appearance (longest first)
  long n_empty = 0;       // rows without stored entries
  char* d_block = nullptr;
  int* d_long_row = nullptr;   // n_long: compact index -> row
  int* d_item_dst = nullptr;   // n_long_items: item -> compact index of its row
  int* d_mrow_dst = nullptr;   // n_mrows: chunked row -> compact index
  int* d_empty_row = nullptr;  // n_empty
};

void free_implicit_lists(ImplicitLists* l) {
  if (!l) return;
  if (l->d_block) (void)hipFree(l->d_block);
  delete l;
}

}  // namespace cumf

namespace {

bool implicit_f_ok(int f) { return f >= 8 && f <= 128 && (f % 2) == 0; }
bool solver_f_ok(int f, int solver) {
  if (solver == CUMF_SOLVER_CG_MATFREE) return matfree_f_ok(f);
  return implicit_f_ok(f) && (solver == CUMF_SOLVER_CG || solver == CUMF_SOLVER_LU);
}

int implicit_lists(cumf_plan* p, ImplicitLists** out) {
  if (p->implicit) {
    *out = p->implicit;
    return 0;
  }
  const size_t ni = (size_t)p->n_items, nm = (size_t)p->n_mrows;
  std::vector<int> row(ni), len(ni), mrow(nm);
  if (ni) {
    CUMF_HIP_CHECK(hipMemcpy(row.data(), p->d_item_row, ni * sizeof(int), hipMemcpyDeviceToHost));
    CUMF_HIP_CHECK(hipMemcpy(len.data(), p->d_item_len, ni * sizeof(int), hipMemcpyDeviceToHost));
  }
  if (nm) CUMF_HIP_CHECK(hipMemcpy(mrow.data(), p->d_mrow_row, nm * sizeof(int), hipMemcpyDeviceToHost));
  const long n_long_items = p->n_items - p->n_short;
  std::vector<int> long_row, item_dst((size_t)n_long_items), mrow_dst(nm), empty;
  std::unordered_map<int, int> dst;
  for (long i = 0; i < n_long_items; ++i) {
    auto it = dst.find(row[i]);
    if (it == dst.end()) {
      it = dst.emplace(row[i], (int)long_row.size()).first;
      long_row.push_back(row[i]);
    }
    item_dst[i] = it->second;
  }
  for (size_t k = 0; k < nm; ++k) mrow_dst[k] = dst.at(mrow[k]);
  for (size_t i = 0; i < ni; ++i)
    if (len[i] == 0) empty.push_back(row[i]);  // an empty row is one whole item of length 0
  std::vector<int> host;
  host.insert(host.end(), long_row.begin(), long_row.end());
  host.insert(host.end(), item_dst.begin(), item_dst.end());
  host.insert(host.end(), mrow_dst.begin(), mrow_dst.end());
  host.insert(host.end(), empty.begin(), empty.end());
  ImplicitLists* l = new ImplicitLists();
  l->n_long_items = n_long_items;
  l->n_long = (long)long_row.size();
  l->n_empty = (long)empty.size();
  if (!host.empty()) {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&l->d_block), host.size() * sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(l->d_block, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      fprintf(stderr, "HIP Error:\nFile = %s\nLine = %d\nReason = %s\n", __FILE__, __LINE__, hipGetErrorString(e));
      free_implicit_lists(l);
      return (int)e;
    }
    int* d = reinterpret_cast<int*>(l->d_block);
    l->d_long_row = d;
    l->d_item_dst = d + long_row.size();
    l->d_mrow_dst = l->d_item_dst + item_dst.size();
    l->d_empty_row = l->d_mrow_dst + mrow_dst.size();
  }
  p->implicit = l;
  *out = l;
  return 0;
}

ImplicitArgs base_implicit_args(const cumf_plan* p, const int* colidx, const float* val, const float* gather, const float* G,
                                int f, float lambda, float alpha, int reg_mode) {
  ImplicitArgs a{};
  a.item_row = p->d_item_row;
  a.item_begin = p->d_item_begin;
  a.item_len = p->d_item_len;
  a.item_slot = p->d_item_slot;
  a.item_rowlen = p->d_item_rowlen;
  a.mrow_row = p->d_mrow_row;
  a.mrow_slot0 = p->d_mrow_slot0;
  a.mrow_nslots = p->d_mrow_nslots;
  a.mrow_rowlen = p->d_mrow_rowlen;
  a.row_begin = p->row_begin;
  a.colidx = colidx;
  a.val = val;
  a.gather = gather;
  a.G = G;
  a.f = f;
  a.lambda = lambda;
  a.alpha = alpha;
  a.reg_mode = reg_mode;
  return a;
}

int check_args(const char* who, const cumf_plan* p, int f, int reg_mode, int max_f = 128) {
  if (!p || f != p->f || !(max_f > 128 ? matfree_f_ok(f) : implicit_f_ok(f)) ||
      (reg_mode != CUMF_IMPLICIT_REG_WEIGHTED && reg_mode != CUMF_IMPLICIT_REG_PLAIN)) {
    fprintf(stderr, "%s: needs a plan of the same f, even 8 <= f <= %d (got %d) and reg_mode 0 or 1 (got %d)\n", who, max_f,
            f, reg_mode);
    return (int)hipErrorInvalidValue;
  }
  return 0;
}

// The route of an implicit half-iteration, decided here only:
//   LU  every row of the plan is materialised (chunked rows through the slot partials) straight into a batch indexed by
//       row - row_begin and solved by the batched LU into `update`;
//   CG  the plan's short whole rows (its last n_short items, at most kShortRow entries) run the Gram-free CG; the other rows
//       are materialised into a compact batch, their warm starts gathered, solved by the batched CG and scattered back.
//   Both then set the rows without stored entries to 0.
//   CG_MATFREE  no system is formed: every row runs the operator-only CG of als_implicit_free.hip (sparse pass over the row's
//       segments, row pass with G v on the matrix pipe and the CG updates), which also sets the empty rows to 0.
struct ImplicitRoute {
  bool materialise_all;  // LU
  bool matfree;          // CG_MATFREE
  long n_short;          // CG: items [n_items - n_short, n_items) on the Gram-free CG
};
ImplicitRoute implicit_route(const cumf_plan* p, int solver) {
  if (solver == CUMF_SOLVER_LU) return ImplicitRoute{true, false, 0};
  if (solver == CUMF_SOLVER_CG_MATFREE) return ImplicitRoute{false, true, 0};
  return ImplicitRoute{false, false, p->n_short};
}

// The matrix-free half-iteration: the driver of als_free.cpp on the implicit kernels, with the scratch kinds of this file.
int update_matfree(cumf_plan* p, const int* colidx, const float* val, const float* gather, const float* G, float* update,
                   float lambda, float alpha, int reg_mode, int cg_iters, hipStream_t s) {
  ImplicitFreeArgs a{};
  a.G = G;
  a.alpha = alpha;
  a.reg_mode = reg_mode;
  return run_matfree(p, &a, colidx, val, gather, update, lambda, cg_iters, kScratchImpTT, kScratchImpSlots, kScratchImpX, s,
                     [&](int step, int steps) { return launch_implicit_free_pass(a, step, steps, s); });
}

}  // namespace

int cumf::plan_empty_rows(cumf_plan* p, const int** rows, long* count) {
  ImplicitLists* l = nullptr;
  const int rc = implicit_lists(p, &l);
  if (rc) return rc;
  *rows = l->d_empty_row;
  *count = l->n_empty;
  return 0;
}

extern "C" int cumf_implicit_available(int f, int solver) { return solver_f_ok(f, solver); }

extern "C" int cumf_implicit_gram(const float* table, long rows, int f, float* G, void* stream) {
  if (!matfree_f_ok(f) || rows < 0 || !G || (rows > 0 && !table)) {
    fprintf(stderr, "cumf_implicit_gram: needs even 8 <= f <= 512 (got %d) and rows >= 0\n", f);
    return (int)hipErrorInvalidValue;
  }
  const hipStream_t s = static_cast<hipStream_t>(stream);
  ScratchLease lease;
  float* part = nullptr;
  int rc = scratch(s, kScratchImpGram, implicit_gram_part_floats(rows, f), &part);
  if (rc) return rc;
  CUMF_HIP_CHECK(launch_implicit_gram(table, rows, f, part, G, nullptr, s));
  return 0;
}

extern "C" int cumf_get_hermitian_implicit(const cumf_plan_t* p, const int* colidx, const float* val, const float* gather,
                                           const float* G, float* tt, float* rhs, int f, float lambda, float alpha,
                                           int reg_mode, void* stream) {
  int rc = check_args("cumf_get_hermitian_implicit", p, f, reg_mode);
  if (rc) return rc;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  ScratchLease lease;
  ImplicitArgs a = base_implicit_args(p, colidx, val, gather, G, f, lambda, alpha, reg_mode);
  a.tt = tt;
  a.rhs = rhs;
  if ((rc = scratch(s, kScratchImpSlots, (size_t)p->n_slots * ((size_t)f * f + f), &a.slots))) return rc;
  CUMF_HIP_CHECK(launch_implicit_hermitian(a, p->n_items, p->n_mrows, s));
  return 0;
}

extern "C" int cumf_get_hermitian_implicit_partial(const cumf_plan_t* p, const int* colidx, const float* val,
                                                   const float* gather, float* packed, float* rhs, int f, float lambda,
                                                   float alpha, int reg_mode, void* stream) {
  int rc = check_args("cumf_get_hermitian_implicit_partial", p, f, reg_mode);
  if (rc) return rc;
  if (!packed || !rhs) {
    fprintf(stderr, "cumf_get_hermitian_implicit_partial: packed and rhs must not be NULL\n");
    return (int)hipErrorInvalidValue;
  }
  const hipStream_t s = static_cast<hipStream_t>(stream);
  ScratchLease lease;
  // the plan lists EVERY row of its batch as an item (a row without entries as one item of length 0), so the item pass itself
  // writes the all-zero partials of the rows that have no entry in this plan: no clearing pass over the batch
  ImplicitArgs a = base_implicit_args(p, colidx, val, gather, nullptr, f, lambda, alpha, reg_mode);
  a.tt = packed;
  a.rhs = rhs;
  if ((rc = scratch(s, kScratchImpSlots, (size_t)p->n_slots * ((size_t)f * f + f), &a.slots))) return rc;
  CUMF_HIP_CHECK(launch_implicit_partial(a, p->n_items, p->n_mrows, s));
  return 0;
}

extern "C" int cumf_implicit_finish(const float* packed, const float* G, float reg_add, float* tt, long batch, int f,
                                    void* stream) {
  if (!implicit_f_ok(f) || batch < 0 || !G || (batch > 0 && (!packed || !tt))) {
    fprintf(stderr, "cumf_implicit_finish: needs even 8 <= f <= 128 (got %d), batch >= 0 and non-NULL buffers\n", f);
    return (int)hipErrorInvalidValue;
  }
  CUMF_HIP_CHECK(launch_implicit_finish(packed, G, reg_add, tt, batch, f, static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int cumf_als_update_implicit(const cumf_plan_t* pc, const int* colidx, const float* val, const float* gather,
                                        const float* G, float* update, int f, float lambda, float alpha, int reg_mode,
                                        int solver, int cg_iters, void* stream) {
  int rc = check_args("cumf_als_update_implicit", pc, f, reg_mode, solver == CUMF_SOLVER_CG_MATFREE ? 512 : 128);
  if (rc) return rc;
  if (!cumf_implicit_available(f, solver)) {
    fprintf(stderr, "cumf_als_update_implicit: unknown solver %d\n", solver);
    return (int)hipErrorInvalidValue;
  }
  cumf_plan* p = const_cast<cumf_plan*>(pc);  // the implicit lists are built on the plan at first use
  ImplicitLists* l = nullptr;
  if ((rc = implicit_lists(p, &l))) return rc;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const ImplicitRoute r = implicit_route(p, solver);
  ScratchLease lease;
  if (r.matfree) return update_matfree(p, colidx, val, gather, G, update, lambda, alpha, reg_mode, cg_iters, s);
  ImplicitArgs a = base_implicit_args(p, colidx, val, gather, G, f, lambda, alpha, reg_mode);
  a.update = update;
  a.cg_iters = cg_iters;
  const size_t ff = (size_t)f * f;
  if ((rc = scratch(s, kScratchImpSlots, (size_t)p->n_slots * (ff + f), &a.slots))) return rc;
  if (r.materialise_all) {
    const long rows = p->row_end - p->row_begin;
    if ((rc = scratch(s, kScratchImpTT, (size_t)rows * ff, &a.tt)) || (rc = scratch(s, kScratchImpRhs, (size_t)rows * f, &a.rhs)))
      return rc;
    CUMF_HIP_CHECK(launch_implicit_hermitian(a, p->n_items, p->n_mrows, s));
    if (rows > 0) {
      rc = cumf_lu_solve_batched(a.tt, a.rhs, update + (size_t)p->row_begin * f, rows, f, stream);
      if (rc) return rc;
    }
  } else {
    const long n = l->n_long;
    if (n > 0) {
      float* xc = nullptr;
      if ((rc = scratch(s, kScratchImpTT, (size_t)n * ff, &a.tt)) || (rc = scratch(s, kScratchImpRhs, (size_t)n * f, &a.rhs)) ||
          (rc = scratch(s, kScratchImpX, (size_t)n * f, &xc)))
        return rc;
      ImplicitArgs al = a;
      al.item_dst = l->d_item_dst;
      al.mrow_dst = l->d_mrow_dst;
      CUMF_HIP_CHECK(launch_implicit_hermitian(al, l->n_long_items, p->n_mrows, s));
      CUMF_HIP_CHECK(launch_implicit_copy_rows(l->d_long_row, n, f, update, xc, false, s));
      rc = cumf_cg_solve_batched(a.tt, xc, a.rhs, n, f, cg_iters, stream);
      if (rc) return rc;
      CUMF_HIP_CHECK(launch_implicit_copy_rows(l->d_long_row, n, f, xc, update, true, s));
    }
    // last, so that cumf_last_kernel_name names it when the plan has short rows
    CUMF_HIP_CHECK(launch_implicit_short_cg(a, p->n_items - r.n_short, r.n_short, s));
  }
  CUMF_HIP_CHECK(launch_implicit_zero_rows(l->d_empty_row, l->n_empty, f, update, s));
  return 0;
}

extern "C" int cumf_implicit_loss(const int* rowptr, const int* colidx, const float* val, const float* XT, const float* thetaT,
                                  long m, long n, int f, float lambda, float alpha, int reg_mode, double* out, void* stream) {
  if (!matfree_f_ok(f) || m < 0 || n < 0 || !out ||
      (reg_mode != CUMF_IMPLICIT_REG_WEIGHTED && reg_mode != CUMF_IMPLICIT_REG_PLAIN)) {
    fprintf(stderr, "cumf_implicit_loss: needs even 8 <= f <= 512 (got %d), m, n >= 0 and reg_mode 0 or 1\n", f);
    return (int)hipErrorInvalidValue;
  }
  const hipStream_t s = static_cast<hipStream_t>(stream);
  ScratchLease lease;
  const size_t ff = (size_t)f * f;
  float* part = nullptr;
  double* aux = nullptr;  // Gx | Gy | loss partials
  int rc = scratch(s, kScratchImpGram, std::max(implicit_gram_part_floats(m, f), implicit_gram_part_floats(n, f)), &part);
  if (!rc) rc = scratch(s, kScratchImpAux, 2 * ff + kImpLossBlocks, &aux);
  if (rc) return rc;
  CUMF_HIP_CHECK(launch_implicit_gram(XT, m, f, part, nullptr, aux, s));
  CUMF_HIP_CHECK(launch_implicit_gram(thetaT, n, f, part, nullptr, aux + ff, s));
  CUMF_HIP_CHECK(launch_implicit_loss(rowptr, colidx, val, XT, thetaT, m, f, lambda, alpha, reg_mode, aux, aux + ff,
                                      aux + 2 * ff, out, s));
  return 0;
}
