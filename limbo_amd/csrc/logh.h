// logh.h — the normal constants and Mills' ratio as a positive continued fraction, for every device form of the acquisition
// family: c2 and 1 / T (cei.hip's log Phi, mes.hip's log t) and log h(z), h = phi + z Phi (cei.hip, nei.hip); the constants also for
// kg.hip and ehvi.hip.  The derivation stands in cei.hip's head.
#pragma once
#include "dev.h"

namespace {
constexpr double LOGH_XC = 3.0;     // the crossover: continued fraction beyond |z| = LOGH_XC
constexpr int LOGH_DEPTH = 60;      // partial quotients of T(x)
constexpr double LOGH_LOG_SQRT2PI = 0.91893853320467274178;
constexpr double LOGH_INV_SQRT2PI = 0.39894228040143267794;
constexpr double LOGH_INV_SQRT2 = 0.70710678118654752440;
} // namespace

// c2(x) = 2 / (x + 3 / (x + ... + LOGH_DEPTH / x)) for x > 0, bottom-up; x = inf: 0
static __device__ __forceinline__ double logh_c2(double x)
{
    double t = x;
#pragma unroll 4
    for (int k = LOGH_DEPTH; k >= 3; --k)
        t = x + (double)k / t;
    return 2.0 / t;
}
// 1 / T(x) = x + c2(x); x = inf: inf
static __device__ __forceinline__ double logh_inv_T(double x)
{
    return x + logh_c2(x);
}

// log h(z) with Phi(z) / h(z) and phi(z) / h(z).  z = -inf: (-inf, inf, inf); z = +inf: (inf, 0, 0); NaN: NaN.
static __device__ __forceinline__ void cei_log_h(double z, double& lh, double& r_Phi, double& r_phi)
{
    if (z < -LOGH_XC) {
        const double x = -z, t = logh_inv_T(x), rinv = x + 1.0 / t; // rinv = 1 / R(x)
        lh = -0.5 * x * x - LOGH_LOG_SQRT2PI - (log(rinv) + log(t));
        r_Phi = t;
        r_phi = rinv * t;
        return;
    }
    const double a = fabs(z);
    const double phi = exp(-0.5 * a * a) * LOGH_INV_SQRT2PI;
    const double Q = 0.5 * erfc(a * LOGH_INV_SQRT2);
    const double fm = Q == 0.0 ? phi : phi - a * Q; // h(-|z|); (inf 0 at |z| = inf)
    const double h = z < 0.0 ? fm : z + fm;
    const double Phi = z < 0.0 ? Q : 1.0 - Q;
    lh = log(h);
    r_Phi = Phi / h;
    r_phi = phi / h;
}
