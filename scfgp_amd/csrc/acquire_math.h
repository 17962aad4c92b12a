// The normal-distribution pieces that acquire.hip (scfgp_acquire) and kg.hip (scfgp_acquire_kg) share: phi, Phi, the tail factor r = h / phi
// and h(g) = g Phi(g) + phi(g) itself.  The tail forms are derived at the top of acquire.hip; tests/acquire_ref.py restates them.
#pragma once
#include <hip/hip_runtime.h>

// the value of a row must not depend on what the compiler chose to fuse: no contraction here or in what follows the include
#pragma clang fp contract(off)

namespace {

constexpr double INV_SQRT2 = 0.70710678118654752440;
constexpr double INV_SQRT_2PI = 0.39894228040143267794;
constexpr double SQRT_2_OVER_PI = 0.79788456080286535588;
constexpr double HALF_LOG_2PI = 0.91893853320467274178;
constexpr double SQRT_PI = 1.77245385090551602730;
constexpr double SQRT_PI_OVER_2 = 1.25331413731550025121;

__device__ __forceinline__ double norm_pdf(double g) { return INV_SQRT_2PI * exp(-0.5 * g * g); }
__device__ __forceinline__ double norm_cdf(double g) { return 0.5 * erfc(-g * INV_SQRT2); }
// r = h / phi for g <= -1; e = erfcx(-g / sqrt 2)
__device__ __forceinline__ double tail_r(double g, double e) {
    if (g < -50.0) {
        const double w = 1.0 / g, w2 = w * w;
        return w2 * (1.0 + w2 * (-3.0 + w2 * (15.0 + w2 * (-105.0 + w2 * 945.0))));
    }
    return 1.0 - SQRT_PI * (-g * INV_SQRT2) * e;
}
// h(g) = g Phi(g) + phi(g), by EI's two branches (acquire_value, kind 2, at sigma = 1)
__device__ __forceinline__ double norm_h(double g) {
    if (g > -1.0) return g * norm_cdf(g) + norm_pdf(g);
    return norm_pdf(g) * tail_r(g, erfcx(-g * INV_SQRT2));
}

}  // namespace
