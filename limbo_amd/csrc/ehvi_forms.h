// ehvi_forms.h — the forms the expected-hypervolume-improvement kernels share (ehvi.hip: two objectives, strips; ehvi3.hip: three,
// boxes): psi and its two partials at a threshold, the product with 0 inf = 0, the difference of two values of a falling psi.
#pragma once
#include <cfloat>

#include "logh.h" // the normal constants

namespace {
struct Ev {
    double psi, Phi, phi;
};
} // namespace

// (psi, Phi, phi) of the belief (mu, s) at the finite threshold t.  z < 0: f = phi + z Phi(z), which loses about z^2 ulps to
// cancellation at large |z| (kg.hip: kg_f); z >= 0: f = z + f(-z).  s = 0: the limit.  A NaN anywhere: NaN.
static __device__ __forceinline__ Ev ehvi_ev(double mu, double s, double t)
{
    Ev e;
    const double d = mu - t;
    if (!(s > 0.0)) {
        if (s != s || d != d || s < 0.0)
            e.psi = e.Phi = e.phi = __longlong_as_double(0x7ff8000000000000LL);
        else {
            e.psi = d > 0.0 ? d : 0.0;
            e.Phi = d > 0.0 ? 1.0 : 0.0;
            e.phi = 0.0;
        }
        return e;
    }
    const double z = d / s;
    if (z != z) {
        e.psi = e.Phi = e.phi = z;
        return e;
    }
    const double a = -fabs(z);
    double fm = 0.0, Q = 0.0, phi = 0.0; // f(-|z|), Phi(-|z|), phi(z); all 0 at |z| = inf
    if (a >= -DBL_MAX) {
        phi = exp(-0.5 * a * a) * LOGH_INV_SQRT2PI;
        Q = 0.5 * erfc(-a * LOGH_INV_SQRT2);
        fm = fmax(phi + a * Q, 0.0);
    }
    e.phi = phi;
    e.Phi = z < 0.0 ? Q : 1.0 - Q;
    e.psi = s * (z < 0.0 ? fm : z + fm);
    return e;
}
// x y, with 0 inf = 0 (a strip of no width under an unbounded height, and the other way round); a NaN factor stays NaN
static __device__ __forceinline__ double ehvi_mul(double x, double y)
{
    const double p = x * y;
    return (p != p && x == x && y == y) ? 0.0 : p;
}
// hi - lo >= 0 of two values of a falling psi; both +inf (mu = +inf): the limit, the width `w` of the interval itself
static __device__ __forceinline__ double ehvi_drop(double hi, double lo, double w)
{
    const double d = hi - lo;
    if (d != d && hi == hi && lo == lo)
        return w;
    return d < 0.0 ? 0.0 : d;
}
