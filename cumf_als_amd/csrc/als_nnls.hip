// als_nnls.hip -- batched non-negative least squares on materialised SPD systems (include/cumf_nnls_capi.h):
//   x = argmin_{x >= 0} 1/2 x^T A x - b^T x,   one workgroup per system (grid-stride over the batch).
//
// Block principal pivoting (Kim & Park, "Fast nonnegative matrix factorization: an active-set-like method and
// comparisons", SIAM J. Sci. Comput. 2011), single right-hand side:
//   F = {i : x_warm_i > 0} (passive), G = the rest (active).  Per step:
//     x_F = A_FF^-1 b_F, x_G = 0          the full f x f system with the G rows and columns replaced by the identity and
//                                         b_G = 0 (SPD), eliminated by the register LU of cumf_lu_solve_batched
//                                         (lu_solve_reg, als_lu_reg.h) through a masking loader; empty F: nothing to solve
//     y_G = (A x - b)_G                    one wave per row, fixed-order butterfly sums
//     V = {i in F : x_i < -tol_x} u {i in G : y_i < -tol}
//   V empty: converged.  Else the full exchange (F <- F xor V) while |V| shrinks, or for at most 3 steps after the last
//   shrink; then Murty's backup rule (only the largest index of V moves) until |V| shrinks again.  Finite and
//   deterministic.
// Tolerances (fp32): s = max|b| + max_i A_ii max_{i in F}|x_i| (max_i A_ii = max|A_ij| for SPD A),
//   tol = f 2^-24 s,  tol_x = tol / max_i A_ii.
// A step whose x_F or y_G is not finite (A not SPD: a zero matrix, NaN) ends the row as not converged and writes x = 0.
// The returned x is max(x_F, 0) on F and 0 on G, so min x >= 0 exactly.  A, b are only read; x is the warm start and the
// result.  Integer statistics only (one atomic pair per workgroup): the result is bit-identical from run to run.
#include <hip/hip_runtime.h>

#include <climits>

#include "als_nnls.h"
#include "als_device.h"
#include "als_lu_reg.h"

namespace cumf {

namespace {

// lu_solve_reg's loader on the masked system: A_FF and b_F where both indices are passive, the identity on G.
template <int NB>
struct MaskedLoad {
  const float* A;
  const float* b;
  const int* pas;  // LDS: 1 = passive
  int f;
  template <typename BI, typename BJ>
  __device__ __forceinline__ float operator()(BI, BJ, int ti, int tj) const {
    constexpr int bi = BI::value, bj = BJ::value;
    const int i = 16 * bi + ti, j = 16 * bj + tj;
    if (i >= f || j > f) return 0.f;
    const bool pi = pas[i] != 0;
    if (j == f) return pi ? b[i] : 0.f;
    if (pi && pas[j]) return A[(size_t)i * f + j];
    return i == j ? 1.f : 0.f;
  }
};

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// LDS of one workgroup: the LU's packed row store (+ reciprocals, zeros), then the BPP state.
template <int NB>
struct NnlsSmem {
  float lu[lu_lds_floats(NB, 16 * NB)];
  float xs[16 * NB];  // LU solution (0 on G)
  float ys[16 * NB];  // y = A x - b on G
  int pas[16 * NB];
  float red[4];
  unsigned long long vmask[2], bad[2], fmask[2];
};

template <int NB>
__global__ __launch_bounds__(kThreads) void nnls_bpp_kernel(const float* __restrict__ A, const float* __restrict__ b,
                                                            float* __restrict__ x, long long batch, int f, int cap,
                                                            unsigned long long* __restrict__ stats) {
  __shared__ __attribute__((aligned(16))) NnlsSmem<NB> sm;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long n_failed = 0, n_fact = 0;  // thread 0's sums over this workgroup's systems
  for (long long sys = blockIdx.x; sys < batch; sys += gridDim.x) {
    const float* As = A + (size_t)sys * f * f;
    const float* bs = b + (size_t)sys * f;
    float* xo = x + (size_t)sys * f;
    // warm start, scales
    if (wave < 2) {
      const bool own = tid < f;
      const float xw = own ? xo[tid] : 0.f;
      const float bv = own ? bs[tid] : 0.f;
      const float dv = own ? As[(size_t)tid * f + tid] : 0.f;
      if (own) sm.pas[tid] = xw > 0.f;
      // fmaxf drops NaN: a non-finite b or diagonal is caught here (the masked LU never reads the diagonal of a G row)
      const unsigned long long fm = __ballot(own && xw > 0.f);
      const unsigned long long nanm = __ballot(own && !(isfinite(bv) && isfinite(dv)));
      const float mb = wave_max(fabsf(bv)), md = wave_max(dv);
      if (lane == 0) {
        sm.red[wave] = mb;
        sm.red[2 + wave] = md;
        sm.fmask[wave] = fm;
        sm.bad[wave] = nanm;
      }
    }
    __syncthreads();
    const float max_b = fmaxf(sm.red[0], sm.red[1]);
    const float max_d = fmaxf(sm.red[2], sm.red[3]);
    unsigned long long F0 = sm.fmask[0], F1 = sm.fmask[1];
    const bool nan_in = (sm.bad[0] | sm.bad[1]) != 0;
    int best = INT_MAX, backup = 3;
    int status = nan_in ? 2 : 1;  // 0 converged, 1 cap reached, 2 not finite
    for (int step = 0; step < cap && !nan_in; ++step) {
      __syncthreads();  // pas / red / masks of the previous step are read by everyone
      const int nF = __popcll(F0) + __popcll(F1);
      if (nF > 0) {
        lu_solve_reg<NB>(MaskedLoad<NB>{As, bs, sm.pas, f}, sm.lu, f, sm.lu + lu_packed_floats(NB), sm.xs, tid);
        ++n_fact;
      } else if (tid < f) {
        sm.xs[tid] = 0.f;
      }
      __syncthreads();
      // y_i = (A x - b)_i on G, one wave per row, x_F read in two fixed halves of the row
      for (int i = wave; i < f; i += 4) {
        if (sm.pas[i]) continue;
        const int j0 = lane, j1 = lane + 64;
        const float* Ai = As + (size_t)i * f;
        float t = (j0 < f && sm.pas[j0]) ? Ai[j0] * sm.xs[j0] : 0.f;
        if (j1 < f && sm.pas[j1]) t = fmaf(Ai[j1], sm.xs[j1], t);
        t = wave_sum(t);
        if (lane == 0) sm.ys[i] = t - bs[i];
      }
      __syncthreads();
      const bool own = wave < 2 && tid < f;
      const bool p = own && sm.pas[tid];
      const float xi = p ? sm.xs[tid] : 0.f, yi = (own && !p) ? sm.ys[tid] : 0.f;
      if (wave < 2) {
        const float mx = wave_max(fabsf(xi));
        if (lane == 0) sm.red[wave] = mx;
      }
      __syncthreads();
      const float s = max_b + max_d * fmaxf(sm.red[0], sm.red[1]);
      const float tol = (float)f * 0x1p-24f * s;
      const float tol_x = max_d > 0.f ? tol / max_d : 0.f;
      if (wave < 2) {
        const float v = p ? xi : yi;
        const unsigned long long vm = __ballot(own && (p ? xi < -tol_x : yi < -tol));
        const unsigned long long bm = __ballot(own && !isfinite(v));
        if (lane == 0) {
          sm.vmask[wave] = vm;
          sm.bad[wave] = bm;
        }
      }
      __syncthreads();
      const unsigned long long V0 = sm.vmask[0], V1 = sm.vmask[1];
      if ((sm.bad[0] | sm.bad[1]) != 0 || !isfinite(tol)) {
        status = 2;
        break;
      }
      const int nV = __popcll(V0) + __popcll(V1);
      if (nV == 0) {
        status = 0;
        break;
      }
      if (step + 1 == cap) break;  // status stays 1: the last iterate, clamped, is returned
      unsigned long long E0 = V0, E1 = V1;  // full exchange
      if (nV < best) {
        best = nV;
        backup = 3;
      } else if (backup > 0) {
        --backup;
      } else {  // Murty: the largest infeasible index alone
        if (V1) {
          E0 = 0;
          E1 = 1ull << (63 - __clzll(V1));
        } else {
          E0 = 1ull << (63 - __clzll(V0));
          E1 = 0;
        }
      }
      F0 ^= E0;
      F1 ^= E1;
      if (own) sm.pas[tid] = (int)(((tid < 64 ? F0 >> tid : F1 >> (tid - 64)) & 1ull));
    }
    if (tid < f) {
      const bool p = sm.pas[tid] != 0;
      xo[tid] = (status == 2 || !p) ? 0.f : fmaxf(sm.xs[tid], 0.f);
    }
    if (tid == 0) n_failed += status != 0;
    __syncthreads();  // pas / xs are rewritten by the next system
  }
  if (tid == 0 && stats) {
    if (n_failed) atomicAdd(stats, n_failed);
    if (n_fact) atomicAdd(stats + 1, n_fact);
  }
}

}  // namespace

hipError_t launch_nnls(const float* A, const float* b, float* x, long batch, int f, int cap, long long* stats,
                       hipStream_t stream) {
  if (batch <= 0) return hipSuccess;
  // grid-stride: at most kNnlsGrid workgroups, each adding its statistics once
  const dim3 grid((unsigned)(batch < kNnlsGrid ? batch : kNnlsGrid)), block(kThreads);
  auto* st = reinterpret_cast<unsigned long long*>(stats);
  return with_nb<1, kNnlsMaxNB>(nb_for_f(f), [&](auto n) {
    return launch_kernel(nnls_bpp_kernel<decltype(n)::value>, grid, block, 0, stream, A, b, x, (long long)batch, f, cap, st);
  });
}

}  // namespace cumf
