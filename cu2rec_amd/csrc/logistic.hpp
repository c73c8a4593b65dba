// sigma and softplus as the logistic trainer (lmf.hip) and the pairwise-ranking trainer (bpr.hip) evaluate them.
#pragma once

#include <hip/hip_runtime.h>

namespace cu2rec {

// never inf / inf: the exponential's argument is <= 0 on both branches.  NaN in, NaN out.
__device__ __forceinline__ float lmf_sigmoid(float s) {
    if (s >= 0.f) return 1.f / (1.f + expf(-s));
    const float e = expf(s);
    return e / (1.f + e);
}

__device__ __forceinline__ double lmf_softplus(double s) { return fmax(s, 0.0) + log1p(exp(-fabs(s))); }

}  // namespace cu2rec
