// als_topk.hip -- the kernels of top-k recommendation and ranking metrics (include/cumf_topk_capi.h; host side als_topk.cpp).
//
// The score of candidate c for query q is the fp32 fmaf chain s = fma(Q[q,j], C[c,j], s) over j = 0, 1, ..., f - 1 from +0;
// v_mfma_f32_16x16x4_f32 issued in increasing j gives exactly those bits (f padded to a multiple of 4 with zeros).  Ranking is
// the total order "higher score first, then lower index", encoded in one 64-bit key per (score, index): larger key = better.
//   topk_score_kernel    on the scoring core of als_score.h: a workgroup owns kTopkQB queries and one slab of the candidates,
//                        which it walks in blocks of kTopkNC (score_item, the exclusion cursor, score_block).  Each lane
//                        filters its eligible scores (score_row, score_eligible) against the query's current k-th score (a
//                        register); survivors go to a per-query buffer, which the owning wave merges into the query's sorted
//                        list (bitonic sort of 256 keys in registers) when it could overflow.  The grid is persistent: one
//                        list + buffer area per workgroup in `work`.  One slab: the lists are the result; else they are
//                        the slab's partial lists;
//   topk_merge_kernel    one wave per query merges the partial lists of the slabs in slab order;
//   topk_metrics_kernel  one wave per query: hits by binary search in the sorted held-out row, then precision / recall / NDCG;
//                        topk_metrics_reduce_kernel sums the per-query values in query order in fp64 (score_column_sum).
// Every result is bit-identical from run to run: no float atomics, and the result of a query does not depend on the slab cut.
#include <hip/hip_runtime.h>

#include "als_device.h"
#include "als_topk.h"
#include "als_score.h"

namespace cumf {

// (no anonymous namespace: cumf_last_kernel_name reports the kernels as cumf::topk_*)

__device__ __forceinline__ topk_key topk_shfl_xor(topk_key v, int d) {
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, d, 64);
  const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), d, 64);
  return ((topk_key)hi << 32) | lo;
}

// The 256 keys of a wave, element e = 64 i + lane in v[i], sorted in descending order (bitonic network).
__device__ __forceinline__ void topk_sort256(topk_key (&v)[4], int lane) {
#pragma unroll
  for (int size = 2; size <= 256; size <<= 1) {
#pragma unroll
    for (int d = size >> 1; d > 0; d >>= 1) {
      if (d >= 64) {
        const int di = d >> 6;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (i & di) continue;
          const int j = i | di;
          const bool desc = ((64 * i + lane) & size) == 0;
          const topk_key a = v[i], b = v[j];
          const bool sw = desc ? a < b : a > b;
          v[i] = sw ? b : a;
          v[j] = sw ? a : b;
        }
      } else {
        const bool lower = (lane & d) == 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const topk_key o = topk_shfl_xor(v[i], d);
          const bool desc = ((64 * i + lane) & size) == 0;
          const bool keep_max = lower == desc;
          v[i] = keep_max ? (v[i] > o ? v[i] : o) : (v[i] < o ? v[i] : o);
        }
      }
    }
  }
}

// The key at element e (wave-uniform) of a sorted wave array.
__device__ __forceinline__ topk_key topk_element(const topk_key (&v)[4], int e) {
  const int i = e >> 6;
  const topk_key r = i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3];
  const unsigned lo = (unsigned)__shfl((int)(unsigned)r, e & 63, 64);
  const unsigned hi = (unsigned)__shfl((int)(unsigned)(r >> 32), e & 63, 64);
  return ((topk_key)hi << 32) | lo;
}

constexpr float kTopkOpen = __builtin_nanf("");  // threshold of a list with fewer than k entries: everything passes

// Merge the buffer of query slot qi into its sorted list (whole wave): list[0, nlist) + buf[0, cnt) -> the best min(k, .)
// of them; the new k-th score becomes the filter threshold.
__device__ __forceinline__ void topk_merge_query(topk_key* __restrict__ list, topk_key* __restrict__ buf, int k, int qi,
                                              int* nlist, int* cnt, float* thr, int lane) {
  const int nl = nlist[qi], nb = cnt[qi];
  topk_key* L = list + (size_t)qi * k;
  topk_key* B = buf + (size_t)qi * kTopkBuf;
  topk_key v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = 64 * i + lane;
    v[i] = e < kTopkMaxK ? (e < nl ? L[e] : 0ull) : (e - kTopkMaxK < nb ? B[e - kTopkMaxK] : 0ull);
  }
  topk_sort256(v, lane);
  const int nn = nl + nb < k ? nl + nb : k;
#pragma unroll
  for (int i = 0; i < 2; ++i) {  // nn <= k <= 128
    const int e = 64 * i + lane;
    if (e < nn) L[e] = v[i];
  }
  const topk_key kth = topk_element(v, k - 1);
  if (lane == 0) {
    nlist[qi] = nn;
    cnt[qi] = 0;
    thr[qi] = nn == k ? topk_key_score(kth) : kTopkOpen;
  }
  topk_wave_sync();
}

template <bool MULTI>  // MULTI: f > kTopkJC, the features in several LDS chunks (query fragments reloaded per chunk)
__global__ __launch_bounds__(kTopkThreads) void topk_score_kernel(const TopkArgs a) {
  __shared__ __attribute__((aligned(16))) float cs[kTopkNC * kTopkPitch];
  __shared__ topk_key xmask[kTopkQB];  // exclusion bits of the current block, per query slot
  __shared__ int cnt[kTopkQB], nlist[kTopkQB];
  __shared__ float thr[kTopkQB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = a.k;
  topk_key* list = a.work + (size_t)blockIdx.x * kTopkQB * (k + kTopkBuf);
  topk_key* buf = list + (size_t)kTopkQB * k;
  float qf[2][kTopkJC / 4];
  for (long long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
    long long wq0, cb, ce;  // first query of this wave; the slab's candidates
    int slab;
    score_item(a, item, wave, &wq0, &slab, &cb, &ce);
    // lanes 0..31: the wave's queries -- list state and the exclusion cursor
    const int qs = kTopkQW * wave + (lane & (kTopkQW - 1));  // query slot of lanes 0..31 (repeated above)
    long long xp = 0, xe = 0;
    if (lane < kTopkQW) {
      cnt[qs] = 0;
      nlist[qs] = 0;
      thr[qs] = kTopkOpen;
      score_excl_begin(a, wq0 + lane, cb, &xp, &xe);
    }
    topk_wave_sync();
    float th[2][4];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int r = 0; r < 4; ++r) th[qt][r] = kTopkOpen;
    if (!MULTI) topk_load_query(qf, a, wq0, 0, a.f, lane);
    for (long long c0 = cb; c0 < ce; c0 += kTopkNC) {
      const int nc = (int)(ce - c0 < kTopkNC ? ce - c0 : kTopkNC);
      if (lane < kTopkQW) xmask[qs] = score_excl_mask(a, &xp, xe, c0, nc);
      f32x4 acc[2][4];
      score_block<MULTI>(acc, qf, cs, a, wq0, c0, nc, lane);
      // filter: above the query's k-th score so far -> its buffer
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const ScoreRow w = score_row(a, wq0, wave, xmask, lane, qt, r);
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) {
            const int cc = 16 * ct + (lane & 15);
            const float s = acc[qt][ct][r];
            if (score_eligible(w, cc, nc, s) && !(s <= th[qt][r])) {  // s > th, or th open (NaN)
              const int at = atomicAdd(&cnt[w.slot], 1);
              buf[(size_t)w.slot * kTopkBuf + at] = topk_make_key(s, (int)(c0 + cc));
            }
          }
        }
      }
      topk_wave_sync();
      // merge the queries whose buffer could overflow in the next block
      unsigned long long full = __ballot(lane < kTopkQW && cnt[qs] > kTopkBuf - kTopkNC);
      if (full) {
        while (full) {
          const int ql = __builtin_ctzll(full);
          full &= full - 1;
          topk_merge_query(list, buf, k, kTopkQW * wave + ql, nlist, cnt, thr, lane);
        }
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
          for (int r = 0; r < 4; ++r) th[qt][r] = thr[kTopkQW * wave + 16 * qt + 4 * (lane >> 4) + r];
      }
    }
    unsigned long long left = __ballot(lane < kTopkQW && cnt[qs] > 0);
    while (left) {
      const int ql = __builtin_ctzll(left);
      left &= left - 1;
      topk_merge_query(list, buf, k, kTopkQW * wave + ql, nlist, cnt, thr, lane);
    }
    // the wave's lists out: the result (one slab) or the slab's partial lists
    for (int ql = 0; ql < kTopkQW; ++ql) {
      const long long q = wq0 + ql;
      if (q >= a.rows) break;
      const int nl = nlist[kTopkQW * wave + ql];
      const topk_key* L = list + (size_t)(kTopkQW * wave + ql) * k;
      for (int e = lane; e < k; e += 64) {
        const topk_key key = e < nl ? L[e] : 0ull;
        if (a.nslab == 1) {
          a.ids[(size_t)q * k + e] = key ? topk_key_id(key) : -1;
          a.scores[(size_t)q * k + e] = key ? topk_key_score(key) : -__builtin_inff();
        } else {
          a.part[((size_t)slab * a.rows + q) * k + e] = key;
        }
      }
    }
    topk_wave_sync();
  }
}

// One wave per query: the partial lists of the slabs merged in slab order into the query's best k.
__global__ __launch_bounds__(kTopkThreads) void topk_merge_kernel(const topk_key* __restrict__ part, long long rows, int k,
                                                                  int nslab, int* __restrict__ ids, float* __restrict__ scores) {
  const int lane = threadIdx.x & 63;
  const long long q = score_wave_query();
  if (q >= rows) return;
  topk_key v[4] = {0ull, 0ull, 0ull, 0ull};
  for (int s = 0; s < nslab; ++s) {
    const topk_key* L = part + ((size_t)s * rows + q) * k;
#pragma unroll
    for (int i = 2; i < 4; ++i) {
      const int e = 64 * (i - 2) + lane;
      v[i] = e < k ? L[e] : 0ull;
    }
    topk_sort256(v, lane);  // the best 128 of (best so far, slab s) in v[0], v[1]
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int e = 64 * i + lane;
    if (e < k) {
      ids[(size_t)q * k + e] = v[i] ? topk_key_id(v[i]) : -1;
      scores[(size_t)q * k + e] = v[i] ? topk_key_score(v[i]) : -__builtin_inff();
    }
  }
}

// ---- ranking metrics

// per query: (counted, precision, recall, ndcg) into part[4 q ..]; a query without relevant held-out entries counts 0
__global__ __launch_bounds__(kTopkThreads) void topk_metrics_kernel(const int* __restrict__ ids, long long rows, int k,
                                                                    const void* rowptr, int rowptr64,
                                                                    const int* __restrict__ colidx,
                                                                    const float* __restrict__ val,
                                                                    double* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const long long q = score_wave_query();
  if (q >= rows) return;
  const long long tb = topk_rowptr(rowptr, rowptr64, q), te = topk_rowptr(rowptr, rowptr64, q + 1);
  double nrel = 0.0;
  for (long long p = tb + lane; p < te; p += 64) nrel += (!val || val[p] > 0.f) ? 1.0 : 0.0;
  nrel = score_wave_sum(nrel);
  double hits = 0.0, dcg = 0.0, idcg = 0.0;
  for (int j = lane; j < k; j += 64) {
    const double gain = 1.0 / log2((double)(j + 2));
    if (j < nrel) idcg += gain;
    const int id = ids[(size_t)q * k + j];
    if (id < 0) continue;
    const long long lo = score_lower_bound(colidx, tb, te, id);
    if (lo < te && colidx[lo] == id && (!val || val[lo] > 0.f)) {
      hits += 1.0;
      dcg += gain;
    }
  }
  hits = score_wave_sum(hits);
  dcg = score_wave_sum(dcg);
  idcg = score_wave_sum(idcg);
  if (lane == 0) {
    double* o = part + 4 * q;
    const bool counted = nrel >= 1.0;
    o[0] = counted ? 1.0 : 0.0;
    o[1] = counted ? hits / k : 0.0;
    o[2] = counted ? hits / nrel : 0.0;
    o[3] = counted ? dcg / idcg : 0.0;
  }
}

// one workgroup sums the four columns in query order (score_column_sum); out = (count, means)
__global__ __launch_bounds__(kTopkThreads) void topk_metrics_reduce_kernel(const double* __restrict__ part, long long rows,
                                                                           double* __restrict__ out) {
  __shared__ double red[kTopkThreads];
  double tot[4];
  for (int c = 0; c < 4; ++c) tot[c] = score_column_sum(part, rows, 4, c, red);
  if (threadIdx.x == 0) {
    const double n = tot[0];
    out[0] = n;
    for (int c = 1; c < 4; ++c) out[c] = n > 0.0 ? tot[c] / n : 0.0;
  }
}

// ---- launchers

int topk_score_occupancy(bool multi) {
  int occ = 0;
  const void* fn = multi ? reinterpret_cast<const void*>(topk_score_kernel<true>)
                         : reinterpret_cast<const void*>(topk_score_kernel<false>);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, kTopkThreads, 0) != hipSuccess || occ < 1) occ = 1;
  return occ;
}

hipError_t launch_topk_score(const TopkArgs& a, long long grid, hipStream_t stream) {
  if (a.f > kTopkJC) return launch_item_kernel(topk_score_kernel<true>, dim3((unsigned)grid), dim3(kTopkThreads), 0, stream, a);
  return launch_item_kernel(topk_score_kernel<false>, dim3((unsigned)grid), dim3(kTopkThreads), 0, stream, a);
}

hipError_t launch_topk_merge(const topk_key* part, long long rows, int k, int nslab, int* ids, float* scores,
                             hipStream_t stream) {
  const long long wgs = (rows + 3) / 4;
  return launch_item_kernel(topk_merge_kernel, dim3((unsigned)wgs), dim3(kTopkThreads), 0, stream, part, rows, k, nslab, ids,
                            scores);
}

hipError_t launch_topk_metrics(const int* ids, long long rows, int k, const void* rowptr, int rowptr64, const int* colidx,
                               const float* val, double* part, double* out, hipStream_t stream) {
  if (rows > 0) {
    const long long wgs = (rows + 3) / 4;
    hipError_t e = launch_item_kernel(topk_metrics_kernel, dim3((unsigned)wgs), dim3(kTopkThreads), 0, stream, ids, rows, k,
                                      rowptr, rowptr64, colidx, val, part);
    if (e != hipSuccess) return e;
  }
  return launch_kernel(topk_metrics_reduce_kernel, dim3(1), dim3(kTopkThreads), 0, stream, (const double*)part, rows, out);
}

}  // namespace cumf
