// als_topk_wide.hip -- top-k for long lists, k up to kTopkWideMaxK (cumf_topk_wide of include/cumf_topk_capi.h; host side
// als_topk.cpp).  Scores, eligibility, the key order and the cut are those of als_topk.hip (the scoring core of als_score.h), so
// a pair (query, candidate) has the same score bits here, in cumf_topk and in cumf_heldout_ranks.  What differs is the selection:
//   topk_wide_score_kernel  the filter of topk_score_kernel (a lane's eligible scores against the query's k-th score in a
//                           register, survivors into the query's buffer of kTopkBuf keys), but the flush sorts the buffer
//                           alone (bitonic network, two keys per lane) and merges it into the sorted list BY RANK: keys are
//                           unique, so the final position of a buffer key is its index in the sorted buffer plus the number
//                           of list keys that rank before it, and the final position of a list key is its index plus the
//                           number of buffer keys that rank before it (one search in the wave's LDS copy of the sorted
//                           buffer).  The list lives in the workgroup's scratch area and is rewritten in place, in chunks of
//                           64 keys from the tail to the head: a list key only moves towards the tail and its displacement
//                           does not decrease with its index, so a chunk's stores land on keys that were loaded already.
//                           Each chunk passes through LDS, where the buffer keys count its keys (one search per chunk, no
//                           dependent loads from the list).  Positions >= k are dropped;
//   topk_wide_merge_kernel  nslab > 1: one wave per query gives every key of every slab's partial list its final position --
//                           its index in its own list plus, for each other slab, the number of that slab's keys that rank
//                           before it -- and scatters the keys at positions < k into ids / scores.  No sort, no dependence on
//                           the slab order; an empty slot is key 0, which ranks after every key, so a short list needs no
//                           length.
// Every result is bit-identical from run to run and does not depend on the cut or on the grid.
#include <hip/hip_runtime.h>

#include "als_device.h"
#include "als_topk.h"
#include "als_score.h"

namespace cumf {

// (no anonymous namespace: cumf_last_kernel_name reports the kernels as cumf::topk_wide_*)

constexpr float kTopkWideOpen = __builtin_nanf("");  // threshold of a list with fewer than k entries: everything passes

__device__ __forceinline__ topk_key topk_wide_shfl_xor(topk_key v, int d) {
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, d, 64);
  const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), d, 64);
  return ((topk_key)hi << 32) | lo;
}

// The 128 keys of a wave, element e = 64 i + lane in v[i], sorted in descending order (bitonic network).
__device__ __forceinline__ void topk_sort128(topk_key (&v)[2], int lane) {
#pragma unroll
  for (int size = 2; size <= 128; size <<= 1) {
#pragma unroll
    for (int d = size >> 1; d > 0; d >>= 1) {
      if (d == 64) {  // size == 128: the last merge, descending throughout
        const topk_key a = v[0], b = v[1];
        v[0] = a < b ? b : a;
        v[1] = a < b ? a : b;
      } else {
        const bool lower = (lane & d) == 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const topk_key o = topk_wide_shfl_xor(v[i], d);
          const bool desc = ((64 * i + lane) & size) == 0;
          const bool keep_max = lower == desc;
          v[i] = keep_max ? (v[i] > o ? v[i] : o) : (v[i] < o ? v[i] : o);
        }
      }
    }
  }
}

// The number of keys of the descending p[0, n) that rank before x (are larger); p may end in empty slots (key 0).
__device__ __forceinline__ int topk_wide_before(const topk_key* p, int n, topk_key x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (p[mid] > x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The same count in N keys of LDS (N a power of two, empty slots at the end): log2(N) + 1 reads, no branch, so that the
// searches of a lane overlap.
template <int N>
__device__ __forceinline__ int topk_wide_before_lds(const topk_key* p, topk_key x) {
  int pos = 0;
#pragma unroll
  for (int s = N >> 1; s > 0; s >>= 1) pos += p[pos + s - 1] > x ? s : 0;
  return pos + (p[pos] > x ? 1 : 0);
}

// Flush the buffer of query slot qi into its sorted list (whole wave): list[0, nlist) + buf[0, cnt) -> the best min(k, .) of
// them, in place; the new k-th score becomes the filter threshold.  sb, lc: the wave's kTopkBuf + 64 keys of LDS.
// One pass over the list in chunks of 64 keys, the last chunk first and the next one loaded ahead.  A chunk's keys take their
// shift from the sorted buffer in sb and move: every store lands at or behind the key's own place, on a key of this chunk
// (loaded: the store waits for the wave's load) or of a later one (moved already).  The chunk also stands in lc, where the
// buffer keys count the list keys that rank before them.  A chunk that no buffer key reaches ends the pass: the keys of all
// chunks before it rank before every buffer key.
__device__ __forceinline__ void topk_wide_flush(topk_key* __restrict__ list, const topk_key* __restrict__ buf, topk_key* sb,
                                                topk_key* lc, int k, int qi, int* nlist, int* cnt, float* thr, int lane) {
  const int nl = nlist[qi], nb = cnt[qi];
  topk_key* L = list + (size_t)qi * k;
  const topk_key* B = buf + (size_t)qi * kTopkBuf;
  int c = (nl - 1) >> 6;
  topk_key next = c >= 0 && 64 * c + lane < nl ? L[64 * c + lane] : 0ull;
  topk_key v[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) v[i] = 64 * i + lane < nb ? B[64 * i + lane] : 0ull;
  topk_sort128(v, lane);
  int bpos[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    sb[64 * i + lane] = v[i];
    bpos[i] = 64 * i + lane;
  }
  const int nn = nl + nb < k ? nl + nb : k;
  for (; c >= 0; --c) {
    const int e = 64 * c + lane;
    const topk_key key = next;
    if (c > 0) next = L[e - 64];  // a whole chunk, and no store of this pass lands in front of chunk c
    lc[lane] = key;
    topk_wave_sync();  // sb (first round) and lc stand
    const int shift = key ? topk_wide_before_lds<kTopkBuf>(sb, key) : 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) bpos[i] += topk_wide_before_lds<64>(lc, v[i]);
    if (shift && e + shift < k) L[e + shift] = key;
    if (key && e + shift == k - 1) thr[qi] = topk_key_score(key);
    const bool reached = __ballot(shift != 0) != 0;
    topk_wave_sync();  // lc is read
    if (!reached) {
#pragma unroll
      for (int i = 0; i < 2; ++i) bpos[i] += 64 * c;
      break;
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if (!v[i]) bpos[i] = k;
    if (bpos[i] < k) L[bpos[i]] = v[i];
    if (bpos[i] == k - 1) thr[qi] = topk_key_score(v[i]);
  }
  if (lane == 0) {
    nlist[qi] = nn;
    cnt[qi] = 0;
    if (nn < k) thr[qi] = kTopkWideOpen;
  }
  topk_wave_sync();
}

template <bool MULTI>  // MULTI: f > kTopkJC, the features in several LDS chunks (query fragments reloaded per chunk)
__global__ __launch_bounds__(kTopkThreads) void topk_wide_score_kernel(const TopkArgs a) {
  __shared__ __attribute__((aligned(16))) float cs[kTopkNC * kTopkPitch];
  __shared__ topk_key xmask[kTopkQB];  // exclusion bits of the current block, per query slot
  __shared__ topk_key sorted[kTopkThreads / 64][kTopkBuf];  // per wave: the sorted buffer of the query it flushes
  __shared__ topk_key chunk[kTopkThreads / 64][64];         // per wave: the list chunk it is moving
  __shared__ int cnt[kTopkQB], nlist[kTopkQB];
  __shared__ float thr[kTopkQB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = a.k;
  topk_key* list = a.work + (size_t)blockIdx.x * kTopkQB * (k + kTopkBuf);
  topk_key* buf = list + (size_t)kTopkQB * k;
  topk_key* sb = sorted[wave];
  topk_key* lc = chunk[wave];
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
      thr[qs] = kTopkWideOpen;
      score_excl_begin(a, wq0 + lane, cb, &xp, &xe);
    }
    topk_wave_sync();
    float th[2][4];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int r = 0; r < 4; ++r) th[qt][r] = kTopkWideOpen;
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
      // flush the queries whose buffer could overflow in the next block
      unsigned long long full = __ballot(lane < kTopkQW && cnt[qs] > kTopkBuf - kTopkNC);
      if (full) {
        while (full) {
          const int ql = __builtin_ctzll(full);
          full &= full - 1;
          topk_wide_flush(list, buf, sb, lc, k, kTopkQW * wave + ql, nlist, cnt, thr, lane);
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
      topk_wide_flush(list, buf, sb, lc, k, kTopkQW * wave + ql, nlist, cnt, thr, lane);
    }
    // the wave's lists out: the result (one slab) or the slab's partial lists, empty slots as key 0
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

// One wave per query: every key of the slabs' partial lists (nslab x rows x k, descending, empty slots 0) to its final place.
__global__ __launch_bounds__(kTopkThreads) void topk_wide_merge_kernel(const topk_key* __restrict__ part, long long rows, int k,
                                                                       int nslab, int* __restrict__ ids,
                                                                       float* __restrict__ scores) {
  const int lane = threadIdx.x & 63;
  const long long q = score_wave_query();
  if (q >= rows) return;
  const size_t pitch = (size_t)rows * k;  // from a slab's list to the next slab's
  const topk_key* P = part + (size_t)q * k;
  // The keys in all lists together, and a cut that spares most of the searches: with j = ceil(k / nslab), every list whose
  // j-th key is at least `cut` holds j keys >= cut, so nslab j >= k keys are, and a key below it has no place among the best k
  // (a list shorter than j gives cut = 0: nothing is spared).
  const int j = (k + nslab - 1) / nslab;
  int total = 0;
  topk_key cut = ~0ull;
  for (int s = lane; s < nslab; s += 64) {
    const topk_key* L = P + (size_t)s * pitch;
    total += topk_wide_before(L, k, 0ull);
    const topk_key kj = L[j - 1];
    cut = kj < cut ? kj : cut;
  }
  total = score_wave_sum(total);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const topk_key o = topk_wide_shfl_xor(cut, d);
    cut = o < cut ? o : cut;
  }
  for (int e = (total < k ? total : k) + lane; e < k; e += 64) {
    ids[(size_t)q * k + e] = -1;
    scores[(size_t)q * k + e] = -__builtin_inff();
  }
  for (int s = 0; s < nslab; ++s) {
    const topk_key* L = P + (size_t)s * pitch;
    for (int e0 = 0; e0 < k; e0 += 64) {
      const int e = e0 + lane;
      const topk_key key = e < k ? L[e] : 0ull;
      const bool live = key != 0ull && key >= cut;
      if (!__ballot(live)) break;  // descending: nothing further in this list either
      if (!live) continue;
      int pos = e;
      for (int t = 0; t < nslab && pos < k; ++t)
        if (t != s) pos += topk_wide_before(P + (size_t)t * pitch, k, key);
      if (pos < k) {
        ids[(size_t)q * k + pos] = topk_key_id(key);
        scores[(size_t)q * k + pos] = topk_key_score(key);
      }
    }
  }
}

// ---- launchers

int topk_wide_score_occupancy(bool multi) {
  int occ = 0;
  const void* fn = multi ? reinterpret_cast<const void*>(topk_wide_score_kernel<true>)
                         : reinterpret_cast<const void*>(topk_wide_score_kernel<false>);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, kTopkThreads, 0) != hipSuccess || occ < 1) occ = 1;
  return occ;
}

hipError_t launch_topk_wide_score(const TopkArgs& a, long long grid, hipStream_t stream) {
  if (a.f > kTopkJC)
    return launch_item_kernel(topk_wide_score_kernel<true>, dim3((unsigned)grid), dim3(kTopkThreads), 0, stream, a);
  return launch_item_kernel(topk_wide_score_kernel<false>, dim3((unsigned)grid), dim3(kTopkThreads), 0, stream, a);
}

hipError_t launch_topk_wide_merge(const topk_key* part, long long rows, int k, int nslab, int* ids, float* scores,
                                  hipStream_t stream) {
  const long long wgs = (rows + 3) / 4;
  return launch_item_kernel(topk_wide_merge_kernel, dim3((unsigned)wgs), dim3(kTopkThreads), 0, stream, part, rows, k, nslab,
                            ids, scores);
}

}  // namespace cumf
