// digamma.hpp — ψ(x) for x > 0 on the device (and, for the host builds of tests/host_emul/, on the host): the one copy that the mixture
// kernels (gmm_kernels.hpp and what includes it) and the hidden Markov model kernels (hmm_kernels.hpp) share.  Recurrence up to x ≥ 6, then
// the asymptotic series to the B_14 term.  Self-contained: no other header of the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace rxhip {

__host__ __device__ __forceinline__ double digamma_dev(double x) {
    double r = 0.0;
    while (x < 6.0) {
        r -= 1.0 / x;
        x += 1.0;
    }
    const double f = 1.0 / (x * x);
    return r + log(x) - 0.5 / x -
           f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (1.0 / 132 - f * (691.0 / 32760 - f / 12))))));
}

// ψ'(x) for x > 0: recurrence up to x ≥ 10, then the asymptotic series to the B_16 term (the first term left out, B_18/x¹⁹ = 55/x¹⁹, is below
// 6e-17 of ψ'(x) there).  Every term of the recurrence is positive: no cancellation, a few ulp over the whole range.
__host__ __device__ __forceinline__ double trigamma_dev(double x) {
    double r = 0.0;
    while (x < 10.0) {
        r += 1.0 / (x * x);
        x += 1.0;
    }
    const double f = 1.0 / (x * x);
    const double tail = f * (1.0 / 6 - f * (1.0 / 30 - f * (1.0 / 42 - f * (1.0 / 30 - f * (5.0 / 66 - f * (691.0 / 2730 - f * (7.0 / 6 - f * (3617.0 / 510))))))));
    return r + (1.0 / x) * (1.0 + 0.5 / x + tail);
}

}  // namespace rxhip
