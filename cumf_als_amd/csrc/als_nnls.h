// als_nnls.h -- non-negative least squares: what als_nnls.hip (kernel) and als_nnls.cpp (host side; include/cumf_nnls_capi.h)
// share.
#ifndef CUMF_ALS_NNLS_H_
#define CUMF_ALS_NNLS_H_

#include "als_internal.h"

namespace cumf {

constexpr int kNnlsMaxF = 128;
constexpr int kNnlsMaxNB = nb_for_f(kNnlsMaxF);  // 9
constexpr int kNnlsGrid = 2048;                  // workgroups of the grid-stride launch
constexpr int kNnlsDefaultItersBase = 16;        // max_iters = 0: 16 + 2 f steps per system
// cap: passive-set steps per system; stats (may be null): [0] += systems not converged, [1] += factorisations
hipError_t launch_nnls(const float* A, const float* b, float* x, long batch, int f, int cap, long long* stats,
                       hipStream_t stream);

}  // namespace cumf

#endif  // CUMF_ALS_NNLS_H_
