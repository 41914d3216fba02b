// als_rank.hip -- the kernels of full-ranking evaluation (include/cumf_rank_capi.h; host side als_rank.cpp): the rank of every
// held-out entry among all eligible candidates, and the metrics of those ranks.  Scores, eligibility and order are those of
// als_topk.hip (als_score.h): the fp32 fmaf chain in increasing j, one 64-bit key per (score, index), larger key = better.
//   rank_threshold_kernel  one thread per held-out entry (q, t): its own score by a VALU fmaf chain -- the bits the MFMA
//                          sequence of the count pass gives the same pair -- and its key; key 0 (and rank -1) when t is outside
//                          [0, ncand), excluded for q, or its score NaN;
//   rank_sort_kernel       one wave per query sorts the row's keys in place in descending order (a bitonic network whose
//                          comparators all point the same way, so a row of any length needs no padding) and counts the
//                          non-zero ones: the query's thresholds;
//   rank_count_kernel      the hot path, on the scoring core of als_score.h as topk_score_kernel is (score_item, the
//                          exclusion cursor, score_block, score_row / score_eligible).  A lane counts its eligible scores
//                          and drops those below its query's lowest threshold (a register); every other score is
//                          located among the query's sorted thresholds by binary search,
//                          b = thresholds with a larger key, and counted in the integer bucket hist[q][b].  A wave keeps the
//                          thresholds and buckets of its kTopkQW queries in LDS when they fit kRankPoolW (the rows are
//                          contiguous) and adds the buckets to the global ones at the end of the slab; a wave whose queries
//                          have more searches and counts in the global arrays;
//   rank_finish_kernel     one wave per query: rank of the j-th threshold = sum_{b <= j} hist[b] - 1 (the entry counted
//                          itself), written at the entry's place in the held-out row;
//   rank_metrics_kernel    one wave per query sorts the ranks of its relevant entries and reduces them to the per-query
//                          values; rank_metrics_reduce_kernel sums those in query order in fp64 (score_column_sum).
// Only integer atomics: every result is bit-identical from run to run and does not depend on the slab cut.
#include <hip/hip_runtime.h>

#include "als_device.h"
#include "als_rank.h"
#include "als_score.h"

namespace cumf {

// (no anonymous namespace: cumf_last_kernel_name reports the kernels as cumf::rank_*)

// The entries [tb, te) of query q, kept inside [0, n_test) whatever the row pointers hold.
__device__ __forceinline__ void rank_row(const void* rp, int is64, long long q, long long n_test, long long* tb, long long* te) {
  long long b = topk_rowptr(rp, is64, q), e = topk_rowptr(rp, is64, q + 1);
  b = b < 0 ? 0 : (b > n_test ? n_test : b);
  e = e < b ? b : (e > n_test ? n_test : e);
  *tb = b;
  *te = e;
}

__global__ __launch_bounds__(kTopkThreads) void rank_threshold_kernel(const RankArgs a) {
  const long long e = (long long)blockIdx.x * kTopkThreads + threadIdx.x;
  if (e >= a.n_test) return;
  if (e < topk_rowptr(a.test_rowptr, a.test_rowptr64, 0) || e >= topk_rowptr(a.test_rowptr, a.test_rowptr64, a.rows)) return;
  long long lo = 0, hi = a.rows - 1;  // the last q with rowptr[q] <= e
  while (lo < hi) {
    const long long mid = lo + ((hi - lo + 1) >> 1);
    if (topk_rowptr(a.test_rowptr, a.test_rowptr64, mid) <= e) lo = mid; else hi = mid - 1;
  }
  const long long q = lo;
  const int t = a.test_colidx[e];
  bool ok = t >= 0 && t < a.ncand;
  if (ok && a.excl_colidx) {
    const long long xe = topk_rowptr(a.excl_rowptr, a.rowptr64, q + 1);
    const long long xl = score_lower_bound(a.excl_colidx, topk_rowptr(a.excl_rowptr, a.rowptr64, q), xe, t);
    ok = !(xl < xe && a.excl_colidx[xl] == t);
  }
  float s = 0.f;
  if (ok) {
    const float* qr = a.Q + (size_t)q * a.f;
    const float* cr = a.C + (size_t)t * a.f;
    for (int j = 0; j < a.f; ++j) s = __builtin_fmaf(qr[j], cr[j], s);
    ok = s == s;
  }
  a.keys[e] = ok ? topk_make_key(s, t) : 0ull;
  a.ranks[e] = -1;  // rank_finish_kernel writes the ranks of the eligible entries
}

// if K[i] < K[j] swap them (i < j): the larger key to the lower index
__device__ __forceinline__ void rank_cex(topk_key* K, int i, int j) {
  const topk_key x = K[i], y = K[j];
  if (x < y) {
    K[i] = y;
    K[j] = x;
  }
}

// K[0, n) in descending order, by one wave.  Every comparator of this form of the bitonic network puts the larger key at the
// lower index, so the positions from n to the next power of two behave as keys below all others that never move: a
// comparator that reaches one is skipped.
__device__ __forceinline__ void rank_sort_row(topk_key* K, int n, int lane) {
  for (long long size = 2; (size >> 1) < n; size <<= 1) {
    const int half = (int)(size >> 1);
    const long long pairs = ((long long)n + size - 1) / size * half;
    for (long long p = lane; p < pairs; p += 64) {  // block [base, base + size): i against its mirror image
      const long long base = (p / half) * size;
      const int off = (int)(p % half);
      const long long j = base + size - 1 - off;
      if (j < n) rank_cex(K, (int)(base + off), (int)j);
    }
    topk_wave_sync();
    for (int d = half >> 1; d > 0; d >>= 1) {
      const long long prs = ((long long)n + 2 * d - 1) / (2 * d) * d;
      for (long long p = lane; p < prs; p += 64) {
        const long long i = (p / d) * 2 * d + p % d;
        if (i + d < n) rank_cex(K, (int)i, (int)(i + d));
      }
      topk_wave_sync();
    }
  }
}

__global__ __launch_bounds__(kTopkThreads) void rank_sort_kernel(const RankArgs a) {
  const int lane = threadIdx.x & 63;
  const long long q = score_wave_query();
  if (q >= a.rows) return;
  long long tb, te;
  rank_row(a.test_rowptr, a.test_rowptr64, q, a.n_test, &tb, &te);
  const int n = (int)(te - tb < 0x7fffffffLL ? te - tb : 0x7fffffffLL);
  rank_sort_row(a.keys + tb, n, lane);
  int nv = 0;
  for (int i = lane; i < n; i += 64) nv += a.keys[tb + i] != 0ull;
  nv = score_wave_sum(nv);
  if (lane == 0) a.nvalid[q] = nv;
}

// Locate key among the nv sorted thresholds T and count it in H: b = thresholds with a larger key; the last bucket (b == nv)
// enters no rank.
template <typename KeyPtr, typename HistPtr>
__device__ __forceinline__ void rank_consume(KeyPtr T, HistPtr H, int nv, topk_key key) {
  int lo = 0, hi = nv;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (T[mid] > key) lo = mid + 1; else hi = mid;
  }
  if (lo < nv) atomicAdd(&H[lo], 1);
}

constexpr int kRankCsBytes = kTopkNC * kTopkPitch * 4;
constexpr size_t kRankLdsBytes = kRankCsBytes + (size_t)kRankPool * 12 + (size_t)kTopkQB * (8 + 8 + 4 + 4 + 4);

template <bool MULTI>  // MULTI: f > kTopkJC, the features in several LDS chunks (query fragments reloaded per chunk)
__global__ __launch_bounds__(kTopkThreads) void rank_count_kernel(const RankArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rank_lds[];
  float* cs = reinterpret_cast<float*>(rank_lds);                                 // the candidate block
  topk_key* pool = reinterpret_cast<topk_key*>(rank_lds + kRankCsBytes);          // kRankPoolW thresholds per wave
  topk_key* xmask = pool + kRankPool;                                             // exclusion bits of the block, per slot
  long long* tglob = reinterpret_cast<long long*>(xmask + kTopkQB);               // first entry of the slot's row
  int* phist = reinterpret_cast<int*>(tglob + kTopkQB);                           // kRankPoolW buckets per wave
  int* tcnt = phist + kRankPool;                                                  // thresholds of the slot's query
  int* tbase = tcnt + kTopkQB;                                                    // its row's place in the wave's pool
  float* tlow = reinterpret_cast<float*>(tbase + kTopkQB);                        // its lowest threshold's score (NaN: none)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  topk_key* wpool = pool + wave * kRankPoolW;
  int* whist = phist + wave * kRankPoolW;
  float qf[2][kTopkJC / 4];
  for (long long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
    long long wq0, cb, ce;  // first query of this wave; the slab's candidates
    int slab;
    score_item(a, item, wave, &wq0, &slab, &cb, &ce);
    // the wave's rows of held-out keys are contiguous: [w0, w1)
    long long w0 = 0, w1 = 0;
    if (wq0 < a.rows) {
      const long long wql = wq0 + kTopkQW < a.rows ? wq0 + kTopkQW : a.rows;
      long long unused;
      rank_row(a.test_rowptr, a.test_rowptr64, wq0, a.n_test, &w0, &unused);
      rank_row(a.test_rowptr, a.test_rowptr64, wql - 1, a.n_test, &unused, &w1);
      if (w1 < w0) w1 = w0;
    }
    const bool in_lds = w1 - w0 <= kRankPoolW;
    const int wlen = in_lds ? (int)(w1 - w0) : 0;
    for (int i = lane; i < wlen; i += 64) {
      wpool[i] = a.keys[w0 + i];
      whist[i] = 0;
    }
    // lanes 0..31: the wave's queries -- thresholds and the exclusion cursor
    const int qs = kTopkQW * wave + (lane & (kTopkQW - 1));  // query slot of lanes 0..31 (repeated above)
    const long long myq = wq0 + lane;
    long long xp = 0, xe = 0;
    if (lane < kTopkQW) {
      long long tb = w0, te = w0;
      int nv = 0;
      if (myq < a.rows) {
        rank_row(a.test_rowptr, a.test_rowptr64, myq, a.n_test, &tb, &te);
        nv = a.nvalid[myq];
        if (nv > te - tb) nv = (int)(te - tb);
        if (in_lds) {  // inside the pool whatever the row pointers hold
          if (tb < w0) tb = w0;
          if (tb > w1) tb = w1;
          if (nv > w1 - tb) nv = (int)(w1 - tb);
        }
      }
      tglob[qs] = tb;
      tbase[qs] = (int)(tb - w0);
      tcnt[qs] = nv;
      tlow[qs] = nv > 0 ? topk_key_score(a.keys[tb + nv - 1]) : __builtin_nanf("");
      score_excl_begin(a, myq, cb, &xp, &xe);
    }
    topk_wave_sync();
    float thl[2][4];
    int nel[2][4];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        thl[qt][r] = tlow[kTopkQW * wave + 16 * qt + 4 * (lane >> 4) + r];
        nel[qt][r] = 0;
      }
    if (!MULTI) topk_load_query(qf, a, wq0, 0, a.f, lane);
    for (long long c0 = cb; c0 < ce; c0 += kTopkNC) {
      const int nc = (int)(ce - c0 < kTopkNC ? ce - c0 : kTopkNC);
      if (lane < kTopkQW) xmask[qs] = score_excl_mask(a, &xp, xe, c0, nc);
      f32x4 acc[2][4];
      score_block<MULTI>(acc, qf, cs, a, wq0, c0, nc, lane);
      // count: every eligible score, and those not below the query's lowest threshold among its thresholds
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const ScoreRow w = score_row(a, wq0, wave, xmask, lane, qt, r);
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) {
            const int cc = 16 * ct + (lane & 15);
            const float s = acc[qt][ct][r];
            if (score_eligible(w, cc, nc, s)) {
              ++nel[qt][r];
              if (s >= thl[qt][r]) {  // false without thresholds (NaN)
                const topk_key key = topk_make_key(s, (int)(c0 + cc));
                if (in_lds)
                  rank_consume(wpool + tbase[w.slot], whist + tbase[w.slot], tcnt[w.slot], key);
                else
                  rank_consume(a.keys + tglob[w.slot], a.hist + tglob[w.slot], tcnt[w.slot], key);
              }
            }
          }
        }
      }
      topk_wave_sync();
    }
    // the slab's eligible candidates and buckets out
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int v = nel[qt][r];
#pragma unroll
        for (int d = 8; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
        const long long q = wq0 + 16 * qt + 4 * (lane >> 4) + r;
        if ((lane & 15) == 0 && q < a.rows && v) atomicAdd(&a.n_eligible[q], v);
      }
    for (int i = lane; i < wlen; i += 64) {
      const int h = whist[i];
      if (h) atomicAdd(&a.hist[w0 + i], h);
    }
    topk_wave_sync();
  }
}

// One wave per query: ranks of its valid thresholds from the prefix sums of the buckets.
__global__ __launch_bounds__(kTopkThreads) void rank_finish_kernel(const RankArgs a) {
  const int lane = threadIdx.x & 63;
  const long long q = score_wave_query();
  if (q >= a.rows) return;
  long long tb, te;
  rank_row(a.test_rowptr, a.test_rowptr64, q, a.n_test, &tb, &te);
  int nv = a.nvalid[q];
  if (nv > te - tb) nv = (int)(te - tb);
  int before = 0;
  for (int i0 = 0; i0 < nv; i0 += 64) {
    const int i = i0 + lane;
    int x = i < nv ? a.hist[tb + i] : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {  // inclusive scan
      const int y = __shfl_up(x, d, 64);
      if (lane >= d) x += y;
    }
    if (i < nv) {
      const int t = topk_key_id(a.keys[tb + i]);
      const long long lo = score_lower_bound(a.test_colidx, tb, te, t);
      if (lo < te && a.test_colidx[lo] == t) a.ranks[lo] = before + x - 1;
    }
    before += __shfl(x, 63, 64);
  }
}

// ---- metrics

// per query into part[q * (kRankCols + 3 n_k) ..]: (counted, auc counted, AUC, MPR numerator, MPR weight, MRR, AP), then
// (precision, recall, NDCG) per cut-off
__global__ __launch_bounds__(kTopkThreads) void rank_metrics_kernel(const int* __restrict__ ranks,
                                                                    const int* __restrict__ n_eligible, long long rows,
                                                                    const void* rowptr, int rowptr64,
                                                                    const float* __restrict__ val, long long n_test,
                                                                    const RankKs ks, topk_key* __restrict__ keys,
                                                                    double* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const long long q = score_wave_query();
  if (q >= rows) return;
  long long tb, te;
  rank_row(rowptr, rowptr64, q, n_test, &tb, &te);
  const int n = (int)(te - tb < 0x7fffffffLL ? te - tb : 0x7fffffffLL);
  // key of entry i: (2^31 - rank, i) for the relevant entries with a rank, 0 for the others: descending keys = ascending ranks
  int p = 0;
  for (int i = lane; i < n; i += 64) {
    const int r = ranks[tb + i];
    const bool in = r >= 0 && (!val || val[tb + i] > 0.f);
    keys[tb + i] = in ? ((topk_key)(0x80000000u - (unsigned)r) << 32) | (unsigned)i : 0ull;
    p += in;
  }
  p = score_wave_sum(p);
  topk_wave_sync();
  rank_sort_row(keys + tb, n, lane);
  const double N = (double)n_eligible[q];
  double excess = 0.0, mprn = 0.0, mprw = 0.0, ap = 0.0;
  for (int i = lane; i < p; i += 64) {
    const topk_key key = keys[tb + i];
    const double r = (double)(0x80000000u - (unsigned)(key >> 32));
    const double w = val ? (double)val[tb + (unsigned)key] : 1.0;
    excess += r - i;
    if (N > 1.0) {
      mprn += w * r / (N - 1.0);
      mprw += w;
    }
    ap += (i + 1) / (r + 1.0);
  }
  excess = score_wave_sum(excess);
  mprn = score_wave_sum(mprn);
  mprw = score_wave_sum(mprw);
  ap = score_wave_sum(ap);
  const int W = kRankCols + 3 * ks.n;
  double* o = part + (size_t)q * W;
  const bool counted = p >= 1;
  if (lane == 0) {
    const bool auc = counted && N > p;
    const double best = counted ? (double)(0x80000000u - (unsigned)(keys[tb] >> 32)) : 0.0;
    o[0] = counted ? 1.0 : 0.0;
    o[1] = auc ? 1.0 : 0.0;
    o[2] = auc ? 1.0 - excess / ((double)p * (N - p)) : 0.0;
    o[3] = mprn;
    o[4] = mprw;
    o[5] = counted ? 1.0 / (1.0 + best) : 0.0;
    o[6] = counted ? ap / p : 0.0;
  }
  for (int c = 0; c < ks.n; ++c) {
    const int k = ks.k[c];
    double hits = 0.0, dcg = 0.0, idcg = 0.0;
    for (int i = lane; i < p; i += 64) {
      const unsigned r = 0x80000000u - (unsigned)(keys[tb + i] >> 32);
      if (r < (unsigned)k) {
        hits += 1.0;
        dcg += 1.0 / log2((double)r + 2.0);
      }
      if (i < k) idcg += 1.0 / log2((double)(i + 2));
    }
    hits = score_wave_sum(hits);
    dcg = score_wave_sum(dcg);
    idcg = score_wave_sum(idcg);
    if (lane == 0) {
      o[kRankCols + 3 * c] = counted ? hits / k : 0.0;
      o[kRankCols + 3 * c + 1] = counted ? hits / p : 0.0;
      o[kRankCols + 3 * c + 2] = counted ? dcg / idcg : 0.0;
    }
  }
}

// one workgroup sums each column in query order (score_column_sum); out = (queries, auc queries, AUC, MPR, MRR, MAP), then (precision, recall, NDCG) per cut-off
__global__ __launch_bounds__(kTopkThreads) void rank_metrics_reduce_kernel(const double* __restrict__ part, long long rows,
                                                                           int n_k, double* __restrict__ out) {
  __shared__ double red[kTopkThreads];
  __shared__ double tot[kRankCols + 3 * kRankMaxK];
  const int W = kRankCols + 3 * n_k;
  for (int c = 0; c < W; ++c) {
    const double s = score_column_sum(part, rows, W, c, red);
    if (threadIdx.x == 0) tot[c] = s;
  }
  if (threadIdx.x == 0) {
    const double n = tot[0], na = tot[1];
    out[0] = n;
    out[1] = na;
    out[2] = na > 0.0 ? tot[2] / na : 0.0;
    out[3] = tot[4] > 0.0 ? tot[3] / tot[4] : 0.0;
    out[4] = n > 0.0 ? tot[5] / n : 0.0;
    out[5] = n > 0.0 ? tot[6] / n : 0.0;
    for (int c = 0; c < 3 * n_k; ++c) out[6 + c] = n > 0.0 ? tot[kRankCols + c] / n : 0.0;
  }
}

// ---- launchers

int rank_count_occupancy(bool multi) {
  int occ = 0;
  const void* fn = multi ? reinterpret_cast<const void*>(rank_count_kernel<true>)
                         : reinterpret_cast<const void*>(rank_count_kernel<false>);
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRankLdsBytes) != hipSuccess) return 1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, kTopkThreads, kRankLdsBytes) != hipSuccess || occ < 1) occ = 1;
  return occ;
}

hipError_t launch_rank_thresholds(const RankArgs& a, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(a.n_eligible, 0, (size_t)a.rows * sizeof(int), stream);
  if (e != hipSuccess) return e;
  if (a.n_test == 0) {
    return hipMemsetAsync(a.nvalid, 0, (size_t)a.rows * sizeof(int), stream);
  }
  e = hipMemsetAsync(a.hist, 0, (size_t)a.n_test * sizeof(int), stream);
  if (e != hipSuccess) return e;
  const long long wgs = (a.n_test + kTopkThreads - 1) / kTopkThreads;
  e = launch_item_kernel(rank_threshold_kernel, dim3((unsigned)wgs), dim3(kTopkThreads), 0, stream, a);
  if (e != hipSuccess) return e;
  return launch_item_kernel(rank_sort_kernel, dim3((unsigned)((a.rows + 3) / 4)), dim3(kTopkThreads), 0, stream, a);
}

hipError_t launch_rank_count(const RankArgs& a, long long grid, hipStream_t stream) {
  if (a.f > kTopkJC)
    return launch_item_kernel(rank_count_kernel<true>, dim3((unsigned)grid), dim3(kTopkThreads), kRankLdsBytes, stream, a);
  return launch_item_kernel(rank_count_kernel<false>, dim3((unsigned)grid), dim3(kTopkThreads), kRankLdsBytes, stream, a);
}

hipError_t launch_rank_finish(const RankArgs& a, hipStream_t stream) {
  return launch_item_kernel(rank_finish_kernel, dim3((unsigned)((a.rows + 3) / 4)), dim3(kTopkThreads), 0, stream, a);
}

hipError_t launch_rank_metrics(const int* ranks, const int* n_eligible, long long rows, const void* rowptr, int rowptr64,
                               const float* val, long long n_test, const RankKs& ks, unsigned long long* keys, double* part,
                               double* out, hipStream_t stream) {
  if (rows > 0) {
    hipError_t e = launch_item_kernel(rank_metrics_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(kTopkThreads), 0, stream,
                                      ranks, n_eligible, rows, rowptr, rowptr64, val, n_test, ks, keys, part);
    if (e != hipSuccess) return e;
  }
  return launch_kernel(rank_metrics_reduce_kernel, dim3(1), dim3(kTopkThreads), 0, stream, (const double*)part, rows, ks.n,
                       out);
}

}  // namespace cumf
