// als_score.h -- the core of the kernels that score a query table against a candidate table (als_topk.hip, als_rank.hip): the
// 64-bit key of the total order "higher score first, then lower index"; the decoding of a persistent-grid item (score_item); a
// query's forward-only exclusion cursor (score_excl_begin, score_excl_mask); the scores of a block of kTopkNC candidates
// (score_block: staging in LDS, query fragments, v_mfma_f32_16x16x4_f32 in increasing feature order -- written here only, so
// a pair (query, candidate) has the same score bits in every kernel); which of them count (score_row, score_eligible); and
// the lower bound, wave sum, wave-per-query index and column sum of the small kernels.  Device code only; included once per
// translation unit.
#ifndef CUMF_ALS_SCORE_H_
#define CUMF_ALS_SCORE_H_

#include <hip/hip_runtime.h>

#include "als_device.h"
#include "als_topk.h"

namespace cumf {

typedef unsigned long long topk_key;

// score -> 32 bits whose unsigned order is the float order (-0 is taken as +0, so equal scores tie on the index)
__device__ __forceinline__ unsigned topk_ord(float s) {
  unsigned u = __float_as_uint(s + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ topk_key topk_make_key(float s, int id) {
  return ((topk_key)topk_ord(s) << 32) | (topk_key)(~(unsigned)id);
}
__device__ __forceinline__ float topk_key_score(topk_key k) {
  const unsigned o = (unsigned)(k >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
__device__ __forceinline__ int topk_key_id(topk_key k) { return (int)~(unsigned)k; }
// key 0 is below every real key (ord(-inf) = 0x007fffff): an empty slot

// Orders this wave's global stores and LDS operations before its following loads (lanes exchange data through both).
__device__ __forceinline__ void topk_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ long long topk_rowptr(const void* rp, int is64, long long i) {
  return is64 ? static_cast<const long long*>(rp)[i] : (long long)static_cast<const int*>(rp)[i];
}

// The first i in [lo, hi) with p[i] >= x (hi: none) of an ascending p.
template <typename X>
__device__ __forceinline__ long long score_lower_bound(const int* __restrict__ p, long long lo, long long hi, X x) {
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (p[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

template <typename T>  // int or double
__device__ __forceinline__ T score_wave_sum(T x) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, 64);
  return x;
}

// The query of this wave in the kernels that give one wave to each query (grids of (rows + 3) / 4 workgroups).
__device__ __forceinline__ long long score_wave_query() {
  return (long long)blockIdx.x * (kTopkThreads / 64) + (threadIdx.x >> 6);
}

// Column c of part (rows x W) summed by one workgroup in a fixed order: thread t sums queries t, t + 256, ... in order, then a
// halving tree over red[kTopkThreads].  The sum is returned in thread 0.
__device__ __forceinline__ double score_column_sum(const double* __restrict__ part, long long rows, int W, int c, double* red) {
  double s = 0.0;
  for (long long q = threadIdx.x; q < rows; q += kTopkThreads) s += part[(size_t)q * W + c];
  __syncthreads();  // the previous column's tree is read
  red[threadIdx.x] = s;
  for (int w = kTopkThreads / 2; w > 0; w >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
  }
  return threadIdx.x == 0 ? red[0] : 0.0;
}

// Stage candidates [c0, c0 + nc) x features [j0, j0 + fc) into cs (kTopkNC rows of kTopkPitch floats).  Within each group of
// 16 features, feature 16 b + 4 t + kq sits at 16 b + 4 kq + t: the lanes of k-group kq read steps 4 b .. 4 b + 3 with one
// 16-byte load.  Zeros beyond nc and up to the next multiple of 16 features.
__device__ __forceinline__ void topk_stage(float* cs, const float* __restrict__ C, int f, long long c0, int nc, int j0, int fc,
                                           bool vec) {
  const int fcp = (fc + 15) & ~15;
  const int groups = fcp >> 2;  // float4 groups per row
  for (int e = threadIdx.x; e < kTopkNC * groups; e += kTopkThreads) {
    const int r = e / groups, g = e - r * groups;
    const int jj = 4 * g;
    float x[4] = {0.f, 0.f, 0.f, 0.f};
    if (r < nc) {
      const float* src = C + (size_t)(c0 + r) * f + j0 + jj;
      if (vec && jj < fc) {
        const float4 w = *reinterpret_cast<const float4*>(src);
        x[0] = w.x, x[1] = w.y, x[2] = w.z, x[3] = w.w;
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) x[t] = jj + t < fc ? src[t] : 0.f;
      }
    }
    float* dst = cs + r * kTopkPitch + 16 * (g >> 2) + (g & 3);
#pragma unroll
    for (int t = 0; t < 4; ++t) dst[4 * t] = x[t];
  }
}

// A lane's query fragments of features [j0, j0 + fc): qf[qt][s] = Q[q][j0 + 4 s + (lane >> 4)], q = 16 qt + (lane & 15) of the
// wave.
__device__ __forceinline__ void topk_load_query(float (&qf)[2][kTopkJC / 4], const ScoreArgs& a, long long wq0, int j0, int fc,
                                                int lane) {
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const long long q = wq0 + 16 * qt + (lane & 15);
    const float* row = a.Q + (size_t)(q < a.rows ? q : 0) * a.f + j0;
#pragma unroll
    for (int s = 0; s < kTopkJC / 4; ++s) {
      const int j = 4 * s + (lane >> 4);
      qf[qt][s] = (q < a.rows && j < fc) ? row[j] : 0.f;
    }
  }
}

// Item of the persistent grid -> the first query of this wave, the slab and its candidates [cb, ce).
__device__ __forceinline__ void score_item(const ScoreArgs& a, long long item, int wave, long long* wq0, int* slab,
                                           long long* cb, long long* ce) {
  const long long qb = item / a.nslab;
  *slab = (int)(item - qb * a.nslab);
  *wq0 = qb * kTopkQB + kTopkQW * wave;
  *cb = (long long)*slab * a.slab_len;
  *ce = *cb + a.slab_len < a.ncand ? *cb + a.slab_len : a.ncand;
}

// The exclusion cursor of query q: [xp, xe) = its excluded candidates >= cb (empty without exclusion or beyond the last query).
__device__ __forceinline__ void score_excl_begin(const ScoreArgs& a, long long q, long long cb, long long* xp, long long* xe) {
  *xp = *xe = 0;
  if (a.excl_colidx && q < a.rows) {
    *xe = topk_rowptr(a.excl_rowptr, a.rowptr64, q + 1);
    *xp = score_lower_bound(a.excl_colidx, topk_rowptr(a.excl_rowptr, a.rowptr64, q), *xe, cb);
  }
}

// Exclusion bits of the block [c0, c0 + nc), bit c - c0 for candidate c: the cursor only moves forward.
__device__ __forceinline__ topk_key score_excl_mask(const ScoreArgs& a, long long* xp, long long xe, long long c0, int nc) {
  topk_key m = 0;
  while (*xp < xe) {
    const int c = a.excl_colidx[*xp];
    if (c >= c0 + nc) break;
    m |= 1ull << (c - c0);
    ++*xp;
  }
  return m;
}

// acc[qt][ct][r] = the score of (query 16 qt + 4 (lane >> 4) + r of the wave, candidate c0 + 16 ct + (lane & 15)): the fp32
// fmaf chain over j = 0, 1, ..., f - 1 from +0.  Whole workgroup (two barriers per chunk of kTopkJC features).  MULTI:
// f > kTopkJC, qf reloaded per chunk; else qf holds the fragments of all features (topk_load_query(qf, a, wq0, 0, a.f, lane)).
template <bool MULTI>
__device__ __forceinline__ void score_block(f32x4 (&acc)[2][4], float (&qf)[2][kTopkJC / 4], float* cs, const ScoreArgs& a,
                                            long long wq0, long long c0, int nc, int lane) {
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
}

// The header of the visit of a lane's 2 x 4 x 4 scores, which each kernel writes as three unrolled loops over (qt, r, ct)
// around its own consumer (a functor, or any function that holds the loops, costs the MULTI kernels 30 VGPRs and their second
// wave per SIMD).  score_row: row (qt, r) of the lane -- the query's slot in the workgroup (kTopkQW wave + its place in the
// wave), whether it exists, its exclusion bits of the block (xmask: per slot).  score_eligible: the pair (row, candidate
// c0 + cc, cc = 16 ct + (lane & 15)) counts -- the candidate is inside the block and not excluded, the score s is not NaN.
struct ScoreRow {
  int slot;
  bool qok;
  topk_key xm;
};
__device__ __forceinline__ ScoreRow score_row(const ScoreArgs& a, long long wq0, int wave, const topk_key* xmask, int lane,
                                              int qt, int r) {
  const int ql = 16 * qt + 4 * (lane >> 4) + r;
  return ScoreRow{kTopkQW * wave + ql, wq0 + ql < a.rows, xmask[kTopkQW * wave + ql]};
}
__device__ __forceinline__ bool score_eligible(const ScoreRow& w, int cc, int nc, float s) {
  return w.qok && cc < nc && s == s && !((w.xm >> cc) & 1ull);
}

}  // namespace cumf

#endif  // CUMF_ALS_SCORE_H_
