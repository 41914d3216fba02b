// Host-only equivalence check: the parent's slice_batched / one_wave_items against the new als_launch.cpp, with the
// kernel files' launchers replaced by recorders.
#include <cstdio>
#include <cstring>
#include <vector>
#include "als_internal.h"
namespace cumf {
struct Call { int kind, nb, mode; bool whole; long n; KernelArgs a; };
std::vector<Call> g_calls;
static void rec(int kind, int nb, int mode, bool whole, long n, const KernelArgs& a) {
  Call c; memset(&c, 0, sizeof c); c.kind = kind; c.nb = nb; c.mode = mode; c.whole = whole; c.n = n; memcpy(&c.a, &a, sizeof a);
  g_calls.push_back(c);
}
template <int NB> hipError_t wave_item_launch(const KernelArgs& a, int mode, const Route&, bool whole, long n, hipStream_t) { rec(0, NB, mode, whole, n, a); return hipSuccess; }
template <int NB> hipError_t slice_reduce_only(const KernelArgs& a, int mode, const Route&, long n, hipStream_t) { rec(1, NB, mode, false, n, a); return hipSuccess; }
template <int NB> hipError_t slice_half_iteration(const KernelArgs& a, int mode, long ni, long nm, hipStream_t) { rec(2, NB, mode, ni > 0, ni + 1000000 * nm, a); return hipSuccess; }
template <int NB> hipError_t slice_solve(const float*, const float*, float*, long, int, int, int, hipStream_t) { return hipSuccess; }
hipError_t launch_short_cg(const KernelArgs& a, long n, hipStream_t) { rec(3, 0, 0, false, n, a); return hipSuccess; }
hipError_t launch_cg_global(const float*, const float*, float*, long, int, int, bool, hipStream_t) { return hipSuccess; }
}
#include "als_launch.cpp"
namespace cumf {
// ---- the parent's code, verbatim but renamed
static hipError_t old_wave_items(const KernelArgs& a, int mode, const Route& r, bool whole, long n_items, hipStream_t stream) {
  return with_nb<2, kMaxWaveNB>(nb_for_f(a.f), [&](auto nb) { return wave_item_launch<nb>(a, mode, r, whole, n_items, stream); });
}
static hipError_t old_one_wave_items(const KernelArgs& a, int mode, const Route& r, const PlanLists& L, hipStream_t stream) {
  KernelArgs aw = a;
  long n_items = L.n_items;
  if (r.chunk_first) {
    aw.item_row = L.w_row, aw.item_begin = L.w_begin, aw.item_len = L.w_len;
    aw.item_slot = nullptr, aw.item_rowlen = L.w_rowlen;
    n_items = L.n_witems;
  }
  if (r.n_short > 0) {
    n_items -= r.n_short;
    KernelArgs as = aw;
    as.item_row += n_items, as.item_begin += n_items, as.item_len += n_items, as.item_rowlen += n_items;
    hipError_t e = launch_short_cg(as, r.n_short, stream);
    if (e != hipSuccess) return e;
  }
  if (r.chunk_first) {
    KernelArgs ac = a;
    ac.item_row = L.c_row, ac.item_begin = L.c_begin, ac.item_len = L.c_len;
    ac.item_slot = L.c_slot, ac.item_rowlen = L.c_rowlen;
    hipError_t e = old_wave_items(ac, mode, r, false, L.n_citems, stream);
    if (e != hipSuccess) return e;
  }
  return old_wave_items(aw, mode, r, r.chunk_first || L.n_mrows == 0, n_items, stream);
}
template <int NB>
hipError_t old_slice_batched(const KernelArgs& a0, int mode, const Route& r, const PlanLists& L, hipStream_t stream) {
  if constexpr (NB < 2) {
    return hipErrorInvalidValue;
  } else {
  hipError_t e = hipSuccess;
  if (L.n_citems > 0) {
    KernelArgs a = a0;
    a.item_row = L.c_row;
    a.item_begin = L.c_begin;
    a.item_len = L.c_len;
    a.item_slot = L.c_slot;
    a.item_rowlen = L.c_rowlen;
    e = wave_item_launch<NB>(a, kModeLU, r, false, L.n_citems, stream);
    if (e != hipSuccess) return e;
    e = slice_reduce_only<NB>(a0, mode, r, L.n_mrows, stream);
    if (e != hipSuccess) return e;
  }
  if (r.whole == kSolveInKernel) {
    if (L.n_witems <= 0) return hipSuccess;
    KernelArgs a = a0;
    a.item_row = L.w_row;
    a.item_begin = L.w_begin;
    a.item_len = L.w_len;
    a.item_rowlen = L.w_rowlen;
    a.item_slot = nullptr;
    a.dense_slots = 0;
    return wave_item_launch<NB>(a, mode, r, false, L.n_witems, stream);
  }
  for (long w0 = 0; w0 < L.n_witems; w0 += L.part2_rows) {
    const long cnt = L.n_witems - w0 < L.part2_rows ? L.n_witems - w0 : L.part2_rows;
    KernelArgs a = a0;
    a.item_row = L.w_row + w0;
    a.item_begin = L.w_begin + w0;
    a.item_len = L.w_len + w0;
    a.item_rowlen = L.w_rowlen + w0;
    a.item_slot = nullptr;
    a.dense_slots = 1;
    a.part = L.part2;
    a.mrow_row = L.w_row + w0;
    a.mrow_rowlen = L.w_rowlen + w0;
    e = wave_item_launch<NB>(a, kModeLU, r, false, cnt, stream);
    if (e != hipSuccess) return e;
    e = slice_reduce_only<NB>(a, mode, r, cnt, stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
  }
}
// the parent's launch_half_iteration without the timing
static hipError_t old_half(const KernelArgs& a, int mode, const Route& r, const PlanLists& L, hipStream_t stream) {
  const int nb = nb_for_f(a.f);
  hipError_t e = hipErrorInvalidValue;
  switch (r.path) {
    case kPathTwoWave:
      e = with_nb<kMaxWaveNB + 1, kMaxNB>(nb, [&](auto n) { return old_slice_batched<n>(a, mode, r, L, stream); });
      break;
    case kPathOneWave: e = old_one_wave_items(a, mode, r, L, stream); break;
    case kPathWorkgroup:
      e = with_nb<1, kMaxNB>(nb, [&](auto n) { return slice_half_iteration<n>(a, mode, L.n_items, 0, stream); });
      break;
    default: break;
  }
  if (e == hipSuccess && r.path != kPathTwoWave && L.n_mrows > 0) {
    e = with_nb<1, kMaxNB>(nb, [&](auto n) {
      return r.path == kPathOneWave ? slice_reduce_only<n>(a, mode, r, L.n_mrows, stream)
                                    : slice_half_iteration<n>(a, mode, 0, L.n_mrows, stream);
    });
  }
  return e;
}
}  // namespace cumf
using namespace cumf;
int main() {
  static int ir[64], il[64], is[64], irl[64], cr[64], cl[64], cs[64], crl[64], wr[64], wl[64], wrl[64], m1[64], m2[64], m3[64], m4[64];
  static long long ib[64], cb[64], wb[64];
  static float part[4], part2[4];
  long cases = 0, bad = 0, launches = 0;
  for (int nb = 1; nb <= kMaxNB; ++nb)
   for (int mode : {kModeCG, kModeLU, kModeMaterialize})
    for (int path : {kPathWorkgroup, kPathOneWave, kPathTwoWave})
     for (int whole : {kSolveInKernel, kSolveTileBuffer})
      for (int chunked : {kSolveReduce, kSolveWaveCG})
       for (int chunk_first = 0; chunk_first < 2; ++chunk_first)
        for (long n_short : {0L, 3L})
         for (long n_c : {0L, 5L})
          for (long n_w : {0L, 7L, 25L})
           for (long p2 : {10L, 25L, 100L}) {
    if ((path == kPathOneWave) != (nb >= 2 && nb <= kMaxWaveNB) && path != kPathWorkgroup) continue;  // what route_for can give
    if (path == kPathTwoWave && nb <= kMaxWaveNB) continue;
    if (n_short > n_w) continue;
    KernelArgs a; memset(&a, 0, sizeof a);
    a.f = 16 * (nb - 1) + (nb == 1 ? 10 : 0);
    a.item_row = ir, a.item_begin = ib, a.item_len = il, a.item_slot = is, a.item_rowlen = irl;
    a.mrow_row = m1, a.mrow_slot0 = m2, a.mrow_nslots = m3, a.mrow_rowlen = m4, a.part = part; a.dense_slots = 7; a.lambda = 0.5f;
    PlanLists L; memset(&L, 0, sizeof L);
    L.n_citems = n_c, L.n_witems = n_w, L.n_items = n_c + n_w, L.n_mrows = n_c ? 2 : 0;
    L.c_row = cr, L.c_len = cl, L.c_slot = cs, L.c_rowlen = crl, L.c_begin = cb, L.w_row = wr, L.w_len = wl, L.w_rowlen = wrl, L.w_begin = wb;
    L.part2 = part2, L.part2_rows = p2, L.n_short = n_short;
    Route r; memset(&r, 0, sizeof r);
    r.path = (Path)path, r.whole = (Solve)whole, r.chunked = (Solve)chunked, r.chunk_first = chunk_first != 0, r.n_short = n_short;
    g_calls.clear();
    hipError_t e0 = old_half(a, mode, r, L, nullptr);
    std::vector<Call> A = g_calls;
    g_calls.clear();
    hipError_t e1 = launch_half_iteration(a, mode, r, L, nullptr);
    ++cases; launches += A.size();
    bool same = e0 == e1 && A.size() == g_calls.size();
    for (size_t i = 0; same && i < A.size(); ++i) same = memcmp(&A[i], &g_calls[i], sizeof(Call)) == 0;
    if (!same) { ++bad; printf("DIFFERENT nb %d mode %d path %d whole %d chunk_first %d n_short %ld n_c %ld n_w %ld p2 %ld: %zu vs %zu launches, status %d vs %d\n", nb, mode, path, whole, chunk_first, n_short, n_c, n_w, p2, A.size(), g_calls.size(), (int)e0, (int)e1); }
  }
  printf("%ld configurations, %ld recorded launches, %ld different\n", cases, launches, bad);
  return bad != 0;
}
