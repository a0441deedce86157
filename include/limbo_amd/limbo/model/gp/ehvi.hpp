// limbo/model/gp/ehvi.hpp — the two-objective expected hypervolume improvement on the host: the strip sum of include/gpe_ehvi.h in
// plain C++, term for term the definition the device kernel sums (limbo_amd/csrc/ehvi.hip), for models that live on the host (below
// Params::gpu::min_n_for_gpu, the empty model, kernels without device code) and for beliefs no engine is at hand for.
#ifndef LIMBO_AMD_MODEL_GP_EHVI_HPP
#define LIMBO_AMD_MODEL_GP_EHVI_HPP
#include <cmath>
#include <cstdint>
#include <limits>

#include <limbo/model/gp/normal.hpp>

namespace limbo_amd {
    namespace ehvi_host {
        struct Ev {
            double psi, Phi, phi;
        };
        /// psi = E[(Y - t)+], Phi = d psi / d mu, phi = d psi / d s of Y ~ N(mu, s^2) at the finite threshold t; s = 0: the limit
        inline Ev ev(double mu, double s, double t)
        {
            const double nan = std::numeric_limits<double>::quiet_NaN();
            const double d = mu - t;
            if (!(s > 0.0)) {
                if (s != s || d != d || s < 0.0)
                    return Ev{nan, nan, nan};
                return Ev{d > 0.0 ? d : 0.0, d > 0.0 ? 1.0 : 0.0, 0.0};
            }
            const double z = d / s;
            if (z != z)
                return Ev{nan, nan, nan};
            const double a = -std::fabs(z);
            double fm = 0.0, Q = 0.0, phi = 0.0;
            if (std::isfinite(a)) {
                phi = std::exp(-0.5 * a * a) * normal::inv_sqrt_2pi;
                Q = 0.5 * std::erfc(-a * normal::inv_sqrt_2);
                fm = std::fmax(phi + a * Q, 0.0);
            }
            return Ev{s * (z < 0.0 ? fm : z + fm), z < 0.0 ? Q : 1.0 - Q, phi};
        }
        inline double mul(double x, double y)
        {
            const double p = x * y;
            return (p != p && x == x && y == y) ? 0.0 : p;
        }
        inline double drop(double hi, double lo, double w)
        {
            const double d = hi - lo;
            if (d != d && hi == hi && lo == lo)
                return w;
            return d < 0.0 ? 0.0 : d;
        }
        /// ehvi and, part != null, part[4] = d/d mu1, d/d s1, d/d mu2, d/d s2 of one candidate over the prepared front (row-major n x 2)
        inline double strip_sum(const double* front, int64_t n, const double* ref, double mu1, double s1, double mu2, double s2, double* part)
        {
            const double inf = std::numeric_limits<double>::infinity();
            double av = 0, am1 = 0, as1 = 0, am2 = 0, as2 = 0;
            Ev p1{0, 0, 0}, p2{0, 0, 0}; // index i - 1
            double lp = ref[0], hp = ref[1];
            for (int64_t i = 0; i <= n + 1; ++i) {
                const double l = i == 0 ? ref[0] : (i <= n ? front[2 * (i - 1)] : inf);
                const double h = i < n ? front[2 * i + 1] : ref[1];
                Ev e1{0, 0, 0}, e2{0, 0, 0};
                if (i <= n) {
                    e1 = ev(mu1, s1, l);
                    e2 = ev(mu2, s2, h);
                }
                if (i >= 1) {
                    const double w = drop(p1.psi, e1.psi, l - lp);
                    av += mul(w, p2.psi);
                    am2 += mul(w, p2.Phi);
                    as2 += mul(w, p2.phi);
                }
                if (i <= n) {
                    const double v = i == 0 ? e2.psi : drop(e2.psi, p2.psi, hp - h);
                    am1 += mul(e1.Phi, v);
                    as1 += mul(e1.phi, v);
                }
                p1 = e1;
                p2 = e2;
                lp = l;
                hp = h;
            }
            if (part) {
                part[0] = am1;
                part[1] = as1;
                part[2] = am2;
                part[3] = as2;
            }
            return av;
        }
        /// the same over M candidates; partials (may be null): M x 4 column-major
        inline void strip_sums(const double* front, int64_t n, const double* ref, const double* mu1, const double* s1, const double* mu2,
            const double* s2, int64_t M, double* ehvi, double* partials)
        {
            for (int64_t m = 0; m < M; ++m) {
                double p[4];
                ehvi[m] = strip_sum(front, n, ref, mu1[m], s1[m], mu2[m], s2[m], partials ? p : nullptr);
                if (partials)
                    for (int k = 0; k < 4; ++k)
                        partials[m + M * k] = p[k];
            }
        }
    } // namespace ehvi_host
} // namespace limbo_amd
#endif
