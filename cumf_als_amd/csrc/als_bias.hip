// als_bias.hip -- the kernels of biased explicit ALS around the fused half-iteration (include/cumf_bias_capi.h; host side
// als_bias.cpp): the residual ratings, the bias columns of the augmented tables, the rows without ratings, prediction, and
// the fp64 SSE / mean in a fixed order.  None of them depends on the feature-block count; compiled once.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "als_bias.h"
#include "als_device.h"

namespace cumf {

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// CUs of the current device (256 when the query fails), for the grids of the streaming kernels
int device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
    cus = 256;
  return cus;
}
// workgroups for `work` threads' worth of elements: enough to cover them, at most 8 per CU (the rest grid-strides)
unsigned stream_grid(long long work, int threads) {
  const long long want = (work + threads - 1) / threads;
  const long long cap = (long long)device_cus() * 8;
  return (unsigned)(want < 1 ? 1 : (want > cap ? cap : want));
}

}  // namespace

// ----------------------------------------------------------------------------------
// Residual ratings r'[e] = (val[e] - mu) - bias[colidx[e]]: bandwidth-bound (12 bytes per rating + the gathered bias, which
// stays in the caches).  Entries [head, head + 4 n4) go as 16-byte loads and one 16-byte store per lane, the `head` entries
// in front and the tail behind as dwords.
// ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kBiasThreads) void bias_residual_kernel(const float* __restrict__ val,
                                                                     const int* __restrict__ colidx,
                                                                     const float* __restrict__ bias, float mu,
                                                                     float* __restrict__ out, long long head, long long n4,
                                                                     long long count) {
  const long long stride = (long long)gridDim.x * kBiasThreads;
  const long long t0 = (long long)blockIdx.x * kBiasThreads + threadIdx.x;
  const f32x4* v4 = reinterpret_cast<const f32x4*>(val + head);
  const i32x4* c4 = reinterpret_cast<const i32x4*>(colidx + head);
  f32x4* o4 = reinterpret_cast<f32x4*>(out + head);
  for (long long i = t0; i < n4; i += stride) {
    const f32x4 v = v4[i];
    const i32x4 c = c4[i];
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (v[k] - mu) - bias[c[k]];
    o4[i] = o;
  }
  const long long body_end = head + 4 * n4;
  const long long edge = head + (count - body_end);  // entries in front of and behind the 16-byte body
  for (long long j = t0; j < edge; j += stride) {
    const long long e = j < head ? j : body_end + (j - head);
    out[e] = (val[e] - mu) - bias[colidx[e]];
  }
}

hipError_t launch_bias_residual(const float* val, const int* colidx, const float* bias, float mu, float* out,
                                long long count, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  const uintptr_t av = reinterpret_cast<uintptr_t>(val), ac = reinterpret_cast<uintptr_t>(colidx),
                  ao = reinterpret_cast<uintptr_t>(out);
  long long head = 0, n4 = 0;
  if ((av & 3) == 0 && (av & 15) == (ac & 15) && (av & 15) == (ao & 15)) {  // aligned alike: one head serves all three
    head = (long long)(((16 - (av & 15)) & 15) / 4);
    if (head > count) head = count;
    n4 = (count - head) / 4;
  }
  const unsigned grid = stream_grid(n4 > 0 ? n4 : count, kBiasThreads);
  return launch_kernel(bias_residual_kernel, dim3(grid), dim3(kBiasThreads), 0, stream, val, colidx, bias, mu, out, head, n4,
                       count);
}

// ----------------------------------------------------------------------------------
// The bias columns of the augmented tables (als_bias.h).  One thread per table row; the two columns of a row share a
// cache line except where a line boundary falls between them.
// ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kBiasThreads) void bias_columns_kernel(int serving, float* __restrict__ gather,
                                                                    const float* __restrict__ gather_bias,
                                                                    long long gather_rows, float* __restrict__ update,
                                                                    float* __restrict__ own_bias, long long row_begin,
                                                                    long long rows, int F, int own, int other, float s) {
  const long long stride = (long long)gridDim.x * kBiasThreads;
  const long long t0 = (long long)blockIdx.x * kBiasThreads + threadIdx.x;
  for (long long i = t0; i < gather_rows; i += stride) {
    float* g = gather + (size_t)i * F;
    g[own] = serving ? 1.f : s;
    g[other] = serving ? gather_bias[i] : 0.f;
  }
  for (long long j = t0; j < rows; j += stride) {
    const long long u = row_begin + j;
    float* x = update + (size_t)u * F;
    if (serving) {
      const float b = x[own] * s;
      own_bias[u] = b;
      x[own] = b;
      x[other] = 1.f;
    } else {
      x[own] = own_bias[u] / s;  // the warm start of the CG; the LU overwrites it
      x[other] = 0.f;
    }
  }
}

hipError_t launch_bias_columns(bool serving, float* gather, const float* gather_bias, long gather_rows, float* update,
                               float* own_bias, long row_begin, long row_end, int F, int own, int other, float s,
                               hipStream_t stream) {
  const long rows = row_end - row_begin;
  const long most = gather_rows > rows ? gather_rows : rows;
  if (most <= 0) return hipSuccess;
  return launch_kernel(bias_columns_kernel, dim3(stream_grid(most, kBiasThreads)), dim3(kBiasThreads), 0, stream,
                       (int)serving, gather, gather_bias, (long long)gather_rows, update, own_bias, (long long)row_begin,
                       (long long)rows, F, own, other, s);
}

// A row without ratings is one item of row length 0 in the plan's list: the fused kernels solve 0 x = 0 there (NaN).  The
// biased model's minimiser for such a row is x = 0, b = 0.  Runs behind the serving pass: column `other` already holds 1.
__global__ __launch_bounds__(kBiasThreads) void bias_empty_rows_kernel(const int* __restrict__ item_row,
                                                                       const int* __restrict__ item_rowlen,
                                                                       long long n_items, float* __restrict__ update,
                                                                       float* __restrict__ own_bias, int F, int other) {
  const long long stride = (long long)gridDim.x * kBiasThreads;
  for (long long k = (long long)blockIdx.x * kBiasThreads + threadIdx.x; k < n_items; k += stride) {
    if (item_rowlen[k] != 0) continue;
    const long long u = item_row[k];
    float* x = update + (size_t)u * F;
    for (int j = 0; j < F; ++j)
      if (j != other) x[j] = 0.f;
    own_bias[u] = 0.f;
  }
}

hipError_t launch_bias_empty_rows(const int* item_row, const int* item_rowlen, long n_items, float* update, float* own_bias,
                                  int F, int other, hipStream_t stream) {
  if (n_items <= 0) return hipSuccess;
  return launch_kernel(bias_empty_rows_kernel, dim3(stream_grid(n_items, kBiasThreads)), dim3(kBiasThreads), 0, stream,
                       item_row, item_rowlen, (long long)n_items, update, own_bias, F, other);
}

// ----------------------------------------------------------------------------------
// Prediction: mu + the fp32 fmaf chain of cumf_topk_capi.h over the two augmented rows (increasing j, from +0).
// ----------------------------------------------------------------------------------
namespace {
__device__ __forceinline__ float bias_chain(const float* __restrict__ q, const float* __restrict__ t, int F) {
  float s = 0.f;
  if ((F & 1) == 0) {  // rows of an even F are 8-byte aligned
    for (int j = 0; j < F; j += 2) {
      const f32x2 a = *reinterpret_cast<const f32x2*>(q + j);
      const f32x2 b = *reinterpret_cast<const f32x2*>(t + j);
      s = fmaf(a[0], b[0], s);
      s = fmaf(a[1], b[1], s);
    }
  } else {
    for (int j = 0; j < F; ++j) s = fmaf(q[j], t[j], s);
  }
  return s;
}
}  // namespace

__global__ __launch_bounds__(kBiasThreads) void bias_predict_kernel(const int* __restrict__ rows, const int* __restrict__ cols,
                                                                    long long count, const float* __restrict__ XA,
                                                                    const float* __restrict__ TA, int F, float mu, float lo,
                                                                    float hi, float* __restrict__ out) {
  const long long stride = (long long)gridDim.x * kBiasThreads;
  for (long long e = (long long)blockIdx.x * kBiasThreads + threadIdx.x; e < count; e += stride) {
    const float p = mu + bias_chain(XA + (size_t)rows[e] * F, TA + (size_t)cols[e] * F, F);
    out[e] = p < lo ? lo : (p > hi ? hi : p);  // a NaN compares false twice and stays
  }
}

hipError_t launch_bias_predict(const int* rows, const int* cols, long long count, const float* XA, const float* TA, int F,
                               float mu, float lo, float hi, float* out, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  return launch_kernel(bias_predict_kernel, dim3(stream_grid(count, kBiasThreads)), dim3(kBiasThreads), 0, stream, rows,
                       cols, count, XA, TA, F, mu, lo, hi, out);
}

// ----------------------------------------------------------------------------------
// fp64 sums in a fixed order: kBiasSumBlocks workgroups of kBiasThreads threads, thread t of the grid takes the entries
// t, t + T, t + 2 T, ... in that order; a workgroup's threads are summed by the same butterfly every time and written to
// part[block]; one workgroup then sums the partials the same way.  No atomics: bit-identical from run to run.
// ----------------------------------------------------------------------------------
namespace {
__device__ __forceinline__ double bias_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < kBiasThreads / 64; ++w) s += red[w];
  return s;
}
}  // namespace

__global__ __launch_bounds__(kBiasThreads) void bias_sum_kernel(const float* __restrict__ val, const int* __restrict__ row,
                                                                const int* __restrict__ col, long long count,
                                                                const float* __restrict__ XA, const float* __restrict__ TA,
                                                                int F, float mu, double* __restrict__ part) {
  __shared__ double red[kBiasThreads / 64];
  const long long stride = (long long)gridDim.x * kBiasThreads;
  double local = 0.0;
  for (long long e = (long long)blockIdx.x * kBiasThreads + threadIdx.x; e < count; e += stride) {
    if (row != nullptr) {
      const float p = mu + bias_chain(XA + (size_t)row[e] * F, TA + (size_t)col[e] * F, F);
      const float d = val[e] - p;
      local += (double)d * (double)d;
    } else {
      local += (double)val[e];
    }
  }
  const double s = bias_block_sum(local, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(kBiasThreads) void bias_sum_final_kernel(const double* __restrict__ part, double divisor,
                                                                      double* __restrict__ out) {
  __shared__ double red[kBiasThreads / 64];
  double local = 0.0;
  for (int k = threadIdx.x; k < kBiasSumBlocks; k += kBiasThreads) local += part[k];
  const double s = bias_block_sum(local, red);
  if (threadIdx.x == 0) *out = s / divisor;
}

hipError_t launch_bias_sum(const float* val, const int* row, const int* col, long long count, const float* XA,
                           const float* TA, int F, float mu, double* part, double* out, hipStream_t stream) {
  if (count <= 0) return hipMemsetAsync(out, 0, sizeof(double), stream);
  hipError_t e = launch_kernel(bias_sum_kernel, dim3(kBiasSumBlocks), dim3(kBiasThreads), 0, stream, val, row, col, count, XA,
                               TA, F, mu, part);
  if (e != hipSuccess) return e;
  const double divisor = row != nullptr ? 1.0 : (double)count;  // the mean: one fp64 division of the sum
  return launch_kernel(bias_sum_final_kernel, dim3(1), dim3(kBiasThreads), 0, stream, (const double*)part, divisor, out);
}

}  // namespace cumf
