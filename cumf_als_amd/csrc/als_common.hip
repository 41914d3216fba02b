// als_common.hip -- the kernels that do not depend on the feature-block count, compiled once: the standalone CG of
// systems too large for the LDS, the RMSE, the packed Gram triangles of the multi-GPU reduction, the train SSE of
// reduced systems and the f16 pre-split of gram mode "fast".
#include <hip/hip_runtime.h>

#include <cstdint>

#include "als_internal.h"
#include "als_device.h"

namespace cumf {

// CG with A streamed from global memory every mat-vec, for f too large for an
// LDS-resident system (f > 128).  One workgroup per system, thread t owns row t
// (blockDim = f rounded up to 64; same shape as cg.cu:36-231, wave64 reductions).
__global__ void cg_global_kernel(const float* __restrict__ A, float* __restrict__ x, const float* __restrict__ b,
                                 int f, int cg_iters, int a_half) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
  float* ps = smem;             // f
  float* red = smem + blockDim.x;  // nwaves
  const float* As = A + (size_t)blockIdx.x * f * f;
  const _Float16* Ah = reinterpret_cast<const _Float16*>(A) + (size_t)blockIdx.x * f * f;  // a_half (cg.cu:253,289)
  float* xs = x + (size_t)blockIdx.x * f;
  const bool own = tid < f;

  auto block_sum = [&](float v) {
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float s = 0.f;
    for (int w = 0; w < nwaves; ++w) s += red[w];
    return s;
  };
  auto matvec = [&]() {
    float s = 0.f;
    if (own) {
      if (a_half)
        for (int j = 0; j < f; ++j) s = fmaf((float)Ah[(size_t)j * f + tid], ps[j], s);
      else
        for (int j = 0; j < f; ++j) s = fmaf(As[(size_t)j * f + tid], ps[j], s);
    }
    return s;
  };

  float xv = own ? xs[tid] : 0.f;
  if (own) ps[tid] = xv;
  __syncthreads();
  float r = own ? (b[(size_t)blockIdx.x * f + tid] - matvec()) : 0.f;
  __syncthreads();
  float p = r;
  if (own) ps[tid] = p;
  float rsold = block_sum(r * r);  // its barriers also publish ps
  for (int iter = 0; iter < cg_iters; ++iter) {
    const float ap = matvec();
    const float pap = block_sum(own ? p * ap : 0.f);
    const float alpha = rsold / pap;
    xv = fmaf(alpha, p, xv);
    r = fmaf(-alpha, ap, r);
    const float rsnew = block_sum(own ? r * r : 0.f);
    if ((double)rsnew < 1e-4) break;
    const float beta = rsnew / rsold;
    rsold = rsnew;
    p = fmaf(beta, p, r);
    __syncthreads();
    if (own) ps[tid] = p;
    __syncthreads();
  }
  if (own) xs[tid] = xv;
}

// ----------------------------------------------------------------------------------
// Sum of squared errors (RMSE kernel + Sasum, als.cu:191-219, 979-991): 16 lanes per
// rating, 8/16-byte gathers of both factor rows, fp64 accumulation across ratings.
// ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void sse_kernel(const float* __restrict__ val, const int* __restrict__ row,
                                                       const int* __restrict__ col, const float* __restrict__ thetaT,
                                                       const float* __restrict__ XT, long long count, int f,
                                                       int surpass_nan, double* __restrict__ out) {
  __shared__ double red[kThreads / 64];
  const int tid = threadIdx.x, sub = tid & 15;
  const long long per_block = kThreads / 16;
  double local = 0.0;
  for (long long base = (long long)blockIdx.x * per_block; base < count; base += (long long)gridDim.x * per_block) {
    const long long i = base + (tid >> 4);
    float e = 0.f;
    if (i < count) {
      const float* th = thetaT + (size_t)col[i] * f;
      const float* xr = XT + (size_t)row[i] * f;
      float s = 0.f;
      int first_nan = f;
      if (surpass_nan) {  // SURPASS_NAN (als.cu:201-211): stop at the first NaN factor entry
        for (int k = sub * 2; k < f; k += 32) {
          const f32x2 a = *reinterpret_cast<const f32x2*>(th + k);
          const f32x2 b = *reinterpret_cast<const f32x2*>(xr + k);
          if ((a[0] != a[0] || b[0] != b[0]) && k < first_nan) first_nan = k;
          if ((a[1] != a[1] || b[1] != b[1]) && k + 1 < first_nan) first_nan = k + 1;
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
          const int other = __shfl_xor(first_nan, o);
          first_nan = other < first_nan ? other : first_nan;
        }
      }
      for (int k = sub * 2; k < f; k += 32) {
        const f32x2 a = *reinterpret_cast<const f32x2*>(th + k);
        const f32x2 b = *reinterpret_cast<const f32x2*>(xr + k);
        if (k < first_nan) s = fmaf(a[0], b[0], s);
        if (k + 1 < first_nan) s = fmaf(a[1], b[1], s);
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
      e = val[i] - s;
    }
    if (sub == 0 && i < count) local += (double)e * (double)e;
  }
  // block reduction in fp64
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) local += __shfl_xor(local, o);
  if ((tid & 63) == 0) red[tid >> 6] = local;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) s += red[w];
    atomicAdd(out, s);
  }
}

// ----------------------------------------------------------------------------------
// Packed upper triangle of a batch of symmetric f x f Grams (row i keeps columns i .. f-1,
// f (f + 1) / 2 floats per system): the payload of the multi-GPU partial-Gram reduction
// (hugewiki.cu:2703-2717 moves the full f x f per GPU; half of it is redundant).
// ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void pack_upper_kernel(const float* __restrict__ full, float* __restrict__ packed,
                                                              int f) {
  const size_t sys = blockIdx.x;
  const float* A = full + sys * (size_t)f * f;
  float* P = packed + sys * (size_t)(f * (f + 1) / 2);
  for (int e = threadIdx.x; e < f * f; e += kThreads) {
    const int i = e / f, j = e - i * f;
    if (j >= i) P[i * f - i * (i - 1) / 2 + (j - i)] = A[e];
  }
}
__global__ __launch_bounds__(kThreads) void unpack_upper_kernel(const float* __restrict__ packed, float* __restrict__ full,
                                                                int f) {
  const size_t sys = blockIdx.x;
  float* A = full + sys * (size_t)f * f;
  const float* P = packed + sys * (size_t)(f * (f + 1) / 2);
  for (int e = threadIdx.x; e < f * f; e += kThreads) {
    const int i = e / f, j = e - i * f;
    const int a = i < j ? i : j, b = i < j ? j : i;
    A[e] = P[a * f - a * (a - 1) / 2 + (b - a)];
  }
}
// ----------------------------------------------------------------------------------
// Train SSE from materialised systems (round 4; the multi-GPU `reduce` scheme, where the Gram batch is reduced across
// ranks and solved by a batched solver): sum_u (r - x_u . t)^2 = sum r^2 - (2 t.b - t^T G t) with G = A - reg I.  One
// workgroup per system adds 2 t.b - t^T A t + reg |t|^2 (fp64) to *out; sum r^2 is a constant of the data.  A is read by
// columns (symmetric: y_j = sum_i A[i][j] t_i, coalesced over j).  Systems with reg < 0 (the caller's mark for "no rating": its solution is NaN) are skipped;
// reg == 0 is a valid system (lambda = 0).
// ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void quadratic_terms_kernel(const float* __restrict__ A, const float* __restrict__ b,
                                                                   const float* __restrict__ x, const float* __restrict__ reg,
                                                                   int f, double* __restrict__ out) {
  __shared__ float xs[256];
  __shared__ double red[kThreads / 64];
  const size_t sys = blockIdx.x;
  const float rg = reg[sys];
  if (!(rg >= 0.f)) return;  // uniform: negative (or NaN) = no rating
  const int tid = threadIdx.x;
  if (tid < f) xs[tid] = x[sys * f + tid];
  __syncthreads();
  double t = 0.0;
  if (tid < f) {
    const float* col = A + sys * (size_t)f * f + tid;
    float y = 0.f;
    for (int i = 0; i < f; ++i) y = fmaf(col[(size_t)i * f], xs[i], y);
    const float xj = xs[tid];
    t = (double)xj * (2.0 * (double)b[sys * f + tid] - (double)y + (double)rg * (double)xj);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
  if ((tid & 63) == 0) red[tid >> 6] = t;
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) sum += red[w];
    atomicAdd(out, sum);
  }
}

// Gram mode "fast": factor table -> (h, l) f16 words of 4096 x (round to nearest even; als_wave.hip
// kArithFast).  Values whose scaled magnitude leaves the f16 range (|x| >= 15.99, +-inf included) are reported
// through *flag (bit 0); NaN entries (rows without ratings) are not.
__global__ __launch_bounds__(256) void presplit_f16x2_kernel(const float* __restrict__ src,
                                                            unsigned* __restrict__ dst, size_t n4, size_t n,
                                                            int* __restrict__ flag) {
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  auto word = [](float x, bool& bad) {
    const float s = x * 4096.0f;
    // NaN is NOT a range violation: rows / columns without ratings carry NaN factors by design (0/0 in CG, a
    // zero pivot in LU: cg.cu:128) and are never gathered; a NaN that IS gathered shows up in the Gram
    // kernel's own probe (bit 1).  +-inf and finite values beyond the f16 range are flagged.
    bad = bad || (__builtin_fabsf(s) >= 65504.0f);
    const _Float16 h = (_Float16)s;
    const _Float16 l = (_Float16)(s - (float)h);
    h2 w = {h, l};
    return __builtin_bit_cast(unsigned, w);
  };
  bool bad = false;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const f32x4 v = reinterpret_cast<const f32x4*>(src)[i];
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    u4 o = {word(v[0], bad), word(v[1], bad), word(v[2], bad), word(v[3], bad)};
    reinterpret_cast<u4*>(dst)[i] = o;
  }
  for (size_t i = 4 * n4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = word(src[i], bad);
  if (bad) atomicOr(flag, 1);
}
hipError_t launch_presplit(const float* src, unsigned* dst, size_t n, int* flag, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const bool aligned = (reinterpret_cast<uintptr_t>(src) % 16 == 0) && (reinterpret_cast<uintptr_t>(dst) % 16 == 0);
  const size_t n4 = aligned ? n / 4 : 0;
  size_t blocks = (n / 4 + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  if (blocks < 1) blocks = 1;
  return launch_kernel(presplit_f16x2_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, src, dst, n4, n, flag);
}

hipError_t launch_pack_upper(const float* full, float* packed, long batch, int f, int unpack, hipStream_t stream) {
  if (batch <= 0) return hipSuccess;
  return launch_kernel(unpack ? unpack_upper_kernel : pack_upper_kernel, dim3((unsigned)batch), dim3(kThreads), 0, stream,
                       full, packed, f);
}

hipError_t launch_quadratic_terms(const float* A, const float* b, const float* x, const float* reg, long batch, int f,
                                  double* out, hipStream_t stream) {
  if (batch <= 0) return hipSuccess;
  if (f > 256) return hipErrorInvalidValue;
  return launch_kernel(quadratic_terms_kernel, dim3((unsigned)batch), dim3(kThreads), 0, stream, A, b, x, reg, f, out);
}

hipError_t launch_sse(const float* val, const int* row, const int* col, const float* thetaT, const float* XT,
                      long count, int f, int surpass_nan, double* out, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(out, 0, sizeof(double), stream);
  if (e != hipSuccess) return e;
  if (count <= 0) return hipSuccess;
  long blocks = (count + 15) / 16;
  if (blocks > 256 * 16) blocks = 256 * 16;
  return launch_kernel(sse_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, val, row, col, thetaT, XT,
                       (long long)count, f, surpass_nan, out);
}

hipError_t launch_cg_global(const float* A, const float* b, float* x, long batch, int f, int cg_iters, bool a_half,
                            hipStream_t stream) {
  const int threads = ((f + 63) / 64) * 64;
  const size_t lds = (threads + 16) * sizeof(float);
  return launch_kernel(cg_global_kernel, dim3((unsigned)batch), dim3(threads), lds, stream, A, x, b, f, cg_iters,
                       (int)a_half);
}

}  // namespace cumf
