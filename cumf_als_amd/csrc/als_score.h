// als_score.h -- what the kernels that score a query table against a candidate table share (als_topk.hip, als_rank.hip): the
// 64-bit key of the total order "higher score first, then lower index", the staging of a block of candidates in LDS and the
// query fragments of v_mfma_f32_16x16x4_f32.  Device code only; included once per translation unit.
#ifndef CUMF_ALS_SCORE_H_
#define CUMF_ALS_SCORE_H_

#include <hip/hip_runtime.h>

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
// wave.  Args: TopkArgs or RankArgs (Q, rows, f).
template <typename Args>
__device__ __forceinline__ void topk_load_query(float (&qf)[2][kTopkJC / 4], const Args& a, long long wq0, int j0, int fc,
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

}  // namespace cumf

#endif  // CUMF_ALS_SCORE_H_
