// als_topk.hip -- the kernels of top-k recommendation and ranking metrics (include/cumf_topk_capi.h; host side als_topk.cpp).
//
// The score of candidate c for query q is the fp32 fmaf chain s = fma(Q[q,j], C[c,j], s) over j = 0, 1, ..., f - 1 from +0;
// v_mfma_f32_16x16x4_f32 issued in increasing j gives exactly those bits (f padded to a multiple of 4 with zeros).  Ranking is
// the total order "higher score first, then lower index", encoded in one 64-bit key per (score, index): larger key = better.
//   topk_score_kernel    a workgroup owns kTopkQB queries (kTopkQW per wave, their fragments in registers) and one slab of the
//                        candidates, which it walks in blocks of kTopkNC staged in LDS.  Each lane filters its scores against
//                        the query's current k-th score (a register), the exclusion bits of the block and NaN; survivors go
//                        to a per-query buffer, which the owning wave merges into the query's sorted list (bitonic sort of
//                        256 keys in registers) when it could overflow.  The grid is persistent: one list + buffer area per
//                        workgroup in `work`.  One slab: the lists are the result; else they are the slab's partial lists;
//   topk_merge_kernel    one wave per query merges the partial lists of the slabs in slab order;
//   topk_metrics_kernel  one wave per query: hits by binary search in the sorted held-out row, then precision / recall / NDCG;
//                        topk_metrics_reduce_kernel sums the per-query values in query order in fp64.
// Every result is bit-identical from run to run: no float atomics, and the result of a query does not depend on the slab cut.
#include <hip/hip_runtime.h>

#include "als_device.h"
#include "als_topk.h"
#include "als_score.h"

namespace cumf {

// (no anonymous namespace: cumf_last_kernel_name reports the kernels as cumf::topk_*)
// the key of the total order, topk_wave_sync, topk_rowptr, topk_stage and topk_load_query: als_score.h

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
    const long long qb = item / a.nslab;
    const int slab = (int)(item - qb * a.nslab);
    const long long wq0 = qb * kTopkQB + kTopkQW * wave;  // first query of this wave
    const long long cb = (long long)slab * a.slab_len;
    const long long ce = cb + a.slab_len < a.ncand ? cb + a.slab_len : a.ncand;
    // lanes 0..31: the wave's queries -- list state and the exclusion cursor (first entry >= cb)
    const int qs = kTopkQW * wave + (lane & (kTopkQW - 1));  // query slot of lanes 0..31 (repeated above)
    const long long myq = wq0 + lane;
    long long xp = 0, xe = 0;
    if (lane < kTopkQW) {
      cnt[qs] = 0;
      nlist[qs] = 0;
      thr[qs] = kTopkOpen;
      if (a.excl_colidx && myq < a.rows) {
        long long lo = topk_rowptr(a.excl_rowptr, a.rowptr64, myq), hi = topk_rowptr(a.excl_rowptr, a.rowptr64, myq + 1);
        xe = hi;
        while (lo < hi) {
          const long long mid = lo + ((hi - lo) >> 1);
          if (a.excl_colidx[mid] < cb) lo = mid + 1; else hi = mid;
        }
        xp = lo;
      }
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
      if (lane < kTopkQW) {  // exclusion bits of [c0, c0 + nc): the cursor only moves forward
        topk_key m = 0;
        while (xp < xe) {
          const int c = a.excl_colidx[xp];
          if (c >= c0 + nc) break;
          m |= 1ull << (c - c0);
          ++xp;
        }
        xmask[qs] = m;
      }
      f32x4 acc[2][4];
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[qt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int j0 = 0; j0 < a.f; j0 += kTopkJC) {
        const int fc = a.f - j0 < kTopkJC ? a.f - j0 : kTopkJC;
        const int nsteps = (fc + 3) >> 2;
        __syncthreads();  // the previous chunk's readers are done with cs
        topk_stage(cs, a.C, a.f, c0, nc, j0, fc, a.vec);
        if (MULTI) topk_load_query(qf, a, wq0, j0, fc, lane);
        __syncthreads();
#pragma unroll
        for (int b = 0; b < kTopkJC / 16; ++b) {
          if (4 * b < nsteps) {
            float4 cv[4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
              cv[ct] = *reinterpret_cast<const float4*>(cs + (16 * ct + (lane & 15)) * kTopkPitch + 16 * b + 4 * (lane >> 4));
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              if (4 * b + t < nsteps) {
                const float cvt[4] = {t == 0 ? cv[0].x : t == 1 ? cv[0].y : t == 2 ? cv[0].z : cv[0].w,
                                      t == 0 ? cv[1].x : t == 1 ? cv[1].y : t == 2 ? cv[1].z : cv[1].w,
                                      t == 0 ? cv[2].x : t == 1 ? cv[2].y : t == 2 ? cv[2].z : cv[2].w,
                                      t == 0 ? cv[3].x : t == 1 ? cv[3].y : t == 2 ? cv[3].z : cv[3].w};
#pragma unroll
                for (int qt = 0; qt < 2; ++qt)
#pragma unroll
                  for (int ct = 0; ct < 4; ++ct)
                    acc[qt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[qt][4 * b + t], cvt[ct], acc[qt][ct], 0, 0, 0);
              }
            }
          }
        }
      }
      // filter: score (query 16 qt + 4 (lane >> 4) + r of the wave, candidate c0 + 16 ct + (lane & 15))
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ql = 16 * qt + 4 * (lane >> 4) + r;
          const bool qok = wq0 + ql < a.rows;
          const topk_key xm = xmask[kTopkQW * wave + ql];
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) {
            const int cc = 16 * ct + (lane & 15);
            const float s = acc[qt][ct][r];
            // !(s <= th): s > th, or th open (NaN); s == s: not NaN
            if (qok && cc < nc && s == s && !(s <= th[qt][r]) && !((xm >> cc) & 1ull)) {
              const int slot = atomicAdd(&cnt[kTopkQW * wave + ql], 1);
              buf[(size_t)(kTopkQW * wave + ql) * kTopkBuf + slot] = topk_make_key(s, (int)(c0 + cc));
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
  const long long q = (long long)blockIdx.x * (kTopkThreads / 64) + (threadIdx.x >> 6);
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

__device__ __forceinline__ double topk_wave_sum(double x) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, 64);
  return x;
}

// per query: (counted, precision, recall, ndcg) into part[4 q ..]; a query without relevant held-out entries counts 0
__global__ __launch_bounds__(kTopkThreads) void topk_metrics_kernel(const int* __restrict__ ids, long long rows, int k,
                                                                    const void* rowptr, int rowptr64,
                                                                    const int* __restrict__ colidx,
                                                                    const float* __restrict__ val,
                                                                    double* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const long long q = (long long)blockIdx.x * (kTopkThreads / 64) + (threadIdx.x >> 6);
  if (q >= rows) return;
  const long long tb = topk_rowptr(rowptr, rowptr64, q), te = topk_rowptr(rowptr, rowptr64, q + 1);
  double nrel = 0.0;
  for (long long p = tb + lane; p < te; p += 64) nrel += (!val || val[p] > 0.f) ? 1.0 : 0.0;
  nrel = topk_wave_sum(nrel);
  double hits = 0.0, dcg = 0.0, idcg = 0.0;
  for (int j = lane; j < k; j += 64) {
    const double gain = 1.0 / log2((double)(j + 2));
    if (j < nrel) idcg += gain;
    const int id = ids[(size_t)q * k + j];
    if (id < 0) continue;
    long long lo = tb, hi = te;
    while (lo < hi) {
      const long long mid = lo + ((hi - lo) >> 1);
      if (colidx[mid] < id) lo = mid + 1; else hi = mid;
    }
    if (lo < te && colidx[lo] == id && (!val || val[lo] > 0.f)) {
      hits += 1.0;
      dcg += gain;
    }
  }
  hits = topk_wave_sum(hits);
  dcg = topk_wave_sum(dcg);
  idcg = topk_wave_sum(idcg);
  if (lane == 0) {
    double* o = part + 4 * q;
    const bool counted = nrel >= 1.0;
    o[0] = counted ? 1.0 : 0.0;
    o[1] = counted ? hits / k : 0.0;
    o[2] = counted ? hits / nrel : 0.0;
    o[3] = counted ? dcg / idcg : 0.0;
  }
}

// one workgroup: thread t sums queries t, t + 256, ... in order, then a fixed tree; out = (count, means)
__global__ __launch_bounds__(kTopkThreads) void topk_metrics_reduce_kernel(const double* __restrict__ part, long long rows,
                                                                           double* __restrict__ out) {
  __shared__ double red[4][kTopkThreads];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long q = threadIdx.x; q < rows; q += kTopkThreads)
#pragma unroll
    for (int c = 0; c < 4; ++c) s[c] += part[4 * q + c];
#pragma unroll
  for (int c = 0; c < 4; ++c) red[c][threadIdx.x] = s[c];
  for (int w = kTopkThreads / 2; w > 0; w >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < w)
#pragma unroll
      for (int c = 0; c < 4; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + w];
  }
  if (threadIdx.x == 0) {
    const double n = red[0][0];
    out[0] = n;
    for (int c = 1; c < 4; ++c) out[c] = n > 0.0 ? red[c][0] / n : 0.0;
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
