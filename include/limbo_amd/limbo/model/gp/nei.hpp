// limbo/model/gp/nei.hpp — noisy expected improvement in the log domain on the host: include/gpe_nei.h in plain C++, function for
// function what the device computes (limbo_amd/csrc/nei.hip, nei.hpp), for models that live on the host (below
// Params::gpu::min_n_for_gpu, the empty model, kernels without device code) and for beliefs no engine is at hand for.
#ifndef LIMBO_AMD_MODEL_GP_NEI_HPP
#define LIMBO_AMD_MODEL_GP_NEI_HPP
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include <limbo/model/gp/host_small.hpp>
#include <limbo/model/gp/normal.hpp>

namespace limbo_amd {
    namespace nei_host {
        /// include/gpe_nei.h's gpe_lognei_values on the host: the same arguments but the handle
        inline void values(int S, const double* fplus, double xi, const double* cmean, int64_t ldm, const double* csd, int64_t M, double* lognei,
            double* terms)
        {
            const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
            std::vector<double> t((size_t)S);
            for (int64_t m = 0; m < M; ++m) {
                const double sd = csd[m];
                const double lsd = std::log(sd);
                double top = -inf;
                bool bad = sd != sd;
                for (int s = 0; s < S; ++s) {
                    const double d = cmean[s + m * ldm] - fplus[s] - xi;
                    double term;
                    if (sd == 0.0)
                        term = d > 0.0 ? std::log(d) : (d != d ? d : -inf);
                    else {
                        double lh, rP, rp;
                        normal::log_h(d / sd, lh, rP, rp);
                        term = lsd + lh;
                    }
                    t[(size_t)s] = term;
                    bad |= term != term;
                    top = std::max(top, term);
                }
                double val = top;
                if (bad)
                    val = nan;
                else if (top != inf && top != -inf) {
                    double sum = 0.0;
                    for (int s = 0; s < S; ++s)
                        sum += std::exp(t[(size_t)s] - top);
                    val = top + std::log(sum) - std::log((double)S);
                }
                lognei[m] = val;
                if (terms)
                    for (int s = 0; s < S; ++s)
                        terms[s + m * (int64_t)S] = bad ? nan : t[(size_t)s];
            }
        }

        /// What the baseline leaves for the candidates: L_b (B x B, column-major) and the S incumbents
        struct Baseline {
            int64_t B = 0;
            int S = 0;
            std::vector<double> Lb, fplus;
        };
        /// Sig: the baseline's covariance (B x B column-major, the kernel without noise, no jitter); mu_b: its complete means (B);
        /// Z: B x S column-major.  Returns 0, or the 1-based first non-positive pivot of Sig + jitter I.
        inline int prepare(const double* Sig, const double* mu_b, int64_t B, double jitter, const double* Z, int S, Baseline& out)
        {
            out.B = B;
            out.S = S;
            out.Lb.assign(Sig, Sig + B * B);
            for (int64_t i = 0; i < B; ++i)
                out.Lb[(size_t)(i + B * i)] += jitter;
            if (const int rc = host_small::llt_lower(out.Lb.data(), B, B))
                return rc;
            out.fplus.assign((size_t)S, -std::numeric_limits<double>::infinity());
            for (int s = 0; s < S; ++s)
                for (int64_t i = 0; i < B; ++i) {
                    double f = 0.0;
                    for (int64_t j = 0; j <= i; ++j)
                        f += out.Lb[(size_t)(i + B * j)] * Z[j + B * s];
                    out.fplus[(size_t)s] = std::max(out.fplus[(size_t)s], mu_b[i] + f);
                }
            return 0;
        }
        /// m candidates against a prepared baseline: C (B x m column-major, ld B) their cross-covariance with the baseline, overwritten
        /// by u = L_b^-1 c; var, mu (m): gpe_query_batch's variance and the complete means.  lognei, cvar (m) and cmean (S x m, ld = S)
        /// may each be null.
        inline void condition(const Baseline& bl, const double* Z, double xi, double* C, const double* var, const double* mu, int64_t m,
            double* lognei, double* cvar, double* cmean)
        {
            const int64_t B = bl.B;
            const int S = bl.S;
            std::vector<double> cm((size_t)S * (size_t)m), sd((size_t)m), val((size_t)m);
            host_small::solve_lower(bl.Lb.data(), B, B, C, m, B);
            for (int64_t q = 0; q < m; ++q) {
                const double* u = C + B * q;
                double ss = 0.0;
                for (int64_t i = 0; i < B; ++i)
                    ss += u[i] * u[i];
                const double v = var[q] - ss;
                if (cvar)
                    cvar[q] = v;
                sd[(size_t)q] = std::sqrt(v > std::numeric_limits<double>::epsilon() ? v : (v != v ? v : 0.0));
                for (int s = 0; s < S; ++s) {
                    double a = 0.0;
                    for (int64_t i = 0; i < B; ++i)
                        a += u[i] * Z[i + B * s];
                    cm[(size_t)(s + (int64_t)S * q)] = mu[q] + a;
                }
            }
            values(S, bl.fplus.data(), xi, cm.data(), S, sd.data(), m, val.data(), nullptr);
            if (lognei)
                std::copy(val.begin(), val.end(), lognei);
            if (cmean)
                std::copy(cm.begin(), cm.end(), cmean);
        }
    } // namespace nei_host
} // namespace limbo_amd
#endif
