// limbo/model/gp/pathwise.hpp — posterior draws as FUNCTIONS of the query point (an addition; not in limbo): pathwise conditioning
// on a random-Fourier-feature prior (include/gpe_pathwise.h for the formulas and the layouts).  What model::GP::sample_paths
// returns: a PathSet that can be evaluated anywhere, with its exact gradient in the point — the continuous, differentiable form of a
// Thompson draw (acqui/thompson.hpp: thompson_paths_batch).
//   spectral_draws   unit-scale frequencies and phases from a seed, by kernel kind
//   HostPaths        the same formulas on the host, for a host-resident model (model/gp/host_small.hpp) and for the prior
//   PathSet          move-only owner of a gpe_paths (device) or a HostPaths
#ifndef LIMBO_AMD_MODEL_GP_PATHWISE_HPP
#define LIMBO_AMD_MODEL_GP_PATHWISE_HPP
#include <cmath>
#include <cstdint>
#include <functional>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include <Eigen/Core>

#include <limbo/model/gp/host_small.hpp>
#include <limbo/model/gp/query_grad.hpp>

#include "../../../../gpe_pathwise.h"

namespace limbo_amd {
    namespace pathwise {
        struct Spectral {
            std::vector<double> Omega0; // R x Dw, row-major
            std::vector<double> phase;  // R, in [0, 2 pi)
        };

        /// Dw: the inputs, plus Lambda's columns for SE-ARD (nk = D + D k + 1 log-parameters)
        inline int freq_dim(int kind, int nk, int D) { return kind == GPE_KERNEL_SE_ARD && D > 0 ? D + ((nk - 1) / D - 1) : D; }

        /// Draws from the kernel family's spectral law at unit length scale, from std::mt19937_64(seed) through
        /// std::normal_distribution in this order: R Dw normals (Omega0, row-major); for Matern-nu 2 nu more per feature, whose
        /// squares sum to u ~ chi^2(2 nu) and scale the row by sqrt(2 nu / u); then R uniforms for the phases.
        inline Spectral spectral_draws(int kind, int R, int Dw, uint64_t seed)
        {
            std::mt19937_64 gen(seed);
            std::normal_distribution<double> nd(0.0, 1.0);
            Spectral sp;
            sp.Omega0.resize((size_t)R * (size_t)Dw);
            for (double& v : sp.Omega0)
                v = nd(gen);
            const int dof = kind == GPE_KERNEL_MATERN52 ? 5 : kind == GPE_KERNEL_MATERN32 ? 3 : 0;
            for (int r = 0; r < R && dof > 0; ++r) {
                double u = 0.0;
                for (int j = 0; j < dof; ++j) {
                    const double z = nd(gen);
                    u += z * z;
                }
                const double sc = std::sqrt((double)dof / u);
                for (int d = 0; d < Dw; ++d)
                    sp.Omega0[(size_t)r * Dw + d] *= sc;
            }
            std::uniform_real_distribution<double> un(0.0, 2.0 * 3.14159265358979323846);
            sp.phase.resize((size_t)R);
            for (double& v : sp.phase)
                v = un(gen);
            return sp;
        }

        /// k(v, x) from (kind, log-theta) as the engine sees them (the value beside query_grad::dk_dv's derivative)
        inline double k_value(int kind, const double* th, int nk, int D, const double* v, const double* x)
        {
            double z = 0.0, sf2;
            if (kind == GPE_KERNEL_SE_ARD) {
                const int k = (nk - 1) / D - 1;
                sf2 = std::exp(2.0 * th[nk - 1]);
                for (int i = 0; i < D; ++i) {
                    const double d = (v[i] - x[i]) * std::exp(-th[i]);
                    z += d * d;
                }
                for (int j = 0; j < k; ++j) {
                    const double* A = th + D * (j + 1);
                    double pr = 0.0;
                    for (int i = 0; i < D; ++i)
                        pr += A[i] * (v[i] - x[i]);
                    z += pr * pr;
                }
            }
            else {
                const double il = std::exp(-th[0]);
                sf2 = std::exp(2.0 * th[1]);
                for (int i = 0; i < D; ++i) {
                    const double d = (v[i] - x[i]) * il;
                    z += d * d;
                }
            }
            if (kind == GPE_KERNEL_SE_ARD || kind == GPE_KERNEL_EXP)
                return sf2 * std::exp(-0.5 * z);
            if (kind == GPE_KERNEL_MATERN52) {
                const double s = std::sqrt(5.0 * z);
                return sf2 * (1.0 + s + (5.0 / 3.0) * z) * std::exp(-s);
            }
            const double s = std::sqrt(3.0 * z);
            return sf2 * (1.0 + s) * std::exp(-s);
        }

        /// The path set on the host.  make(): omega from Omega0 and the hyper-parameters, U from the factor L (n x n, column-major;
        /// n = 0: the prior's paths).  Layouts: gpe_pathwise.h.
        struct HostPaths {
            int kind = 0, nk = 0, D = 0, P = 0, R = 0, S = 0;
            int64_t n = 0;
            std::vector<double> th, X, omega, phase, W, U; // X: n x D row-major; omega: R x D row-major; W: amp W, R x S P; U: n x S P

            void make(int kind_, const double* th_, int nk_, int D_, int P_, const double* Xrm, int64_t n_, const double* L, const double* obs_mean,
                double noise, int R_, int S_, const double* Omega0, const double* phase_, const double* W_, const double* E)
            {
                kind = kind_, nk = nk_, D = D_, P = P_, R = R_, S = S_, n = n_;
                th.assign(th_, th_ + nk);
                X.assign(Xrm, Xrm + n * D);
                phase.assign(phase_, phase_ + R);
                const int ncols = S * P, Dw = freq_dim(kind, nk, D);
                omega.assign((size_t)R * D, 0.0);
                for (int r = 0; r < R; ++r)
                    for (int d = 0; d < D; ++d) {
                        double o = Omega0[(size_t)r * Dw + d] * std::exp(-th[kind == GPE_KERNEL_SE_ARD ? d : 0]);
                        for (int j = 0; j < Dw - D; ++j)
                            o += th[D * (j + 1) + d] * Omega0[(size_t)r * Dw + D + j];
                        omega[(size_t)r * D + d] = o;
                    }
                const double sf2 = std::exp(2.0 * th[kind == GPE_KERNEL_SE_ARD ? nk - 1 : 1]), amp = std::sqrt(2.0 * sf2 / R);
                W.resize((size_t)R * ncols);
                for (size_t q = 0; q < W.size(); ++q)
                    W[q] = amp * W_[q];
                U.assign((size_t)n * ncols, 0.0);
                if (n == 0)
                    return;
                const double sn = std::sqrt(noise + 1e-8);
                std::vector<double> cs((size_t)R);
                for (int64_t i = 0; i < n; ++i) {
                    for (int r = 0; r < R; ++r)
                        cs[(size_t)r] = std::cos(angle(r, X.data() + i * D));
                    for (int c = 0; c < ncols; ++c) {
                        double f = 0.0;
                        for (int r = 0; r < R; ++r)
                            f += cs[(size_t)r] * W[(size_t)r + (size_t)R * c];
                        U[(size_t)(i + n * c)] = obs_mean[i + n * (c / S)] - f - (E ? sn * E[i + n * c] : 0.0);
                    }
                }
                host_small::solve_lower(L, n, n, U.data(), ncols, n);
                host_small::solve_lower_t(L, n, n, U.data(), ncols, n);
            }
            double angle(int r, const double* x) const
            {
                double a = phase[(size_t)r];
                for (int d = 0; d < D; ++d)
                    a += omega[(size_t)r * D + d] * x[d];
                return a;
            }
            /// F[t + T c] (may be null), dF[t + T (d + D c)] (may be null); mean_q[t + T p] or null
            void eval(const double* Xq, int64_t T, const double* mean_q, double* F, double* dF) const
            {
                const int ncols = S * P;
                std::vector<double> cs((size_t)R), sn((size_t)R), kv((size_t)n), dk((size_t)n * D);
                for (int64_t t = 0; t < T; ++t) {
                    const double* x = Xq + t * D;
                    for (int r = 0; r < R; ++r) {
                        const double a = angle(r, x);
                        cs[(size_t)r] = std::cos(a);
                        sn[(size_t)r] = std::sin(a);
                    }
                    for (int64_t i = 0; i < n; ++i) {
                        kv[(size_t)i] = k_value(kind, th.data(), nk, D, x, X.data() + i * D);
                        if (dF)
                            query_grad::dk_dv(kind, th.data(), nk, D, x, X.data() + i * D, dk.data() + i * D);
                    }
                    for (int c = 0; c < ncols; ++c) {
                        const double* w = W.data() + (size_t)R * c;
                        const double* u = U.data() + (size_t)n * c;
                        if (F) {
                            double a = 0.0, b = 0.0;
                            for (int r = 0; r < R; ++r)
                                a += cs[(size_t)r] * w[r];
                            for (int64_t i = 0; i < n; ++i)
                                b += kv[(size_t)i] * u[i];
                            F[t + T * c] = ((mean_q ? mean_q[t + T * (c / S)] : 0.0) + a) + b;
                        }
                        for (int d = 0; d < D && dF; ++d) {
                            double a = 0.0, b = 0.0;
                            for (int r = 0; r < R; ++r)
                                a -= sn[(size_t)r] * omega[(size_t)r * D + d] * w[r];
                            for (int64_t i = 0; i < n; ++i)
                                b += dk[(size_t)i * D + d] * u[i];
                            dF[t + T * (d + (int64_t)D * c)] = a + b;
                        }
                    }
                }
            }
        };

        /// A set of pathwise posterior draws of a model::GP (GP::sample_paths): draw s of output p is column s + n_draws p.
        /// Move-only; owns the device's gpe_paths or the host data.  A snapshot of the model's samples, kernel and observations at
        /// the time it was made; the MEAN FUNCTOR is evaluated when a point is (mean::NullFunction, Constant: no difference; a mean
        /// that reads the model reads it as it then is), so the model must outlive the set.
        class PathSet {
        public:
            using mean_fn = std::function<Eigen::VectorXd(const Eigen::VectorXd&)>;
            PathSet() = default;
            PathSet(gpe_paths ps, int D, int P, int S, mean_fn mean) : _ps(ps), _D(D), _P(P), _S(S), _mean(std::move(mean)) {}
            PathSet(HostPaths&& hp, mean_fn mean) : _host(std::move(hp)), _D(_host.D), _P(_host.P), _S(_host.S), _mean(std::move(mean)) {}
            PathSet(const PathSet&) = delete;
            PathSet& operator=(const PathSet&) = delete;
            PathSet(PathSet&& o) noexcept { _swap(o); }
            PathSet& operator=(PathSet&& o) noexcept
            {
                if (this != &o) {
                    _release();
                    _swap(o);
                }
                return *this;
            }
            ~PathSet() { _release(); }

            int n_draws() const { return _S; }
            int dim_in() const { return _D; }
            int dim_out() const { return _P; }
            bool on_device() const { return _ps != nullptr; }

            /// per draw a T x dim_out matrix, the mean functor added
            std::vector<Eigen::MatrixXd> eval(const std::vector<Eigen::VectorXd>& points) const
            {
                std::vector<Eigen::MatrixXd> F;
                _eval(points, &F, nullptr);
                return F;
            }
            /// F as eval(); dF[s + n_draws p] is T x dim_in: row t = d f_sp / d x at points[t] (without the mean functor's derivative)
            void eval_grad(const std::vector<Eigen::VectorXd>& points, std::vector<Eigen::MatrixXd>& F, std::vector<Eigen::MatrixXd>& dF) const
            {
                _eval(points, &F, &dF);
            }
            /// idx[s + n_draws p], fmax[s + n_draws p]: the maximiser of every draw over the points, the lowest index on exact ties
            void argmax(const std::vector<Eigen::VectorXd>& points, std::vector<int64_t>& idx, std::vector<double>& fmax) const
            {
                const int64_t T = points.size();
                idx.assign((size_t)(_S * _P), 0);
                fmax.assign((size_t)(_S * _P), 0.0);
                if (T == 0)
                    return;
                std::vector<double> Xq, mq;
                _stage(points, Xq, mq);
                if (_ps) {
                    _check(gpe_paths_argmax(_ps, Xq.data(), T, mq.data(), idx.data(), fmax.data()), "gpe_paths_argmax");
                    return;
                }
                std::vector<double> F((size_t)(T * _S * _P));
                _host.eval(Xq.data(), T, mq.data(), F.data(), nullptr);
                for (int c = 0; c < _S * _P; ++c) {
                    int64_t best = 0;
                    for (int64_t t = 1; t < T; ++t)
                        if (F[(size_t)(t + T * c)] > F[(size_t)(best + T * c)])
                            best = t;
                    idx[(size_t)c] = best;
                    fmax[(size_t)c] = F[(size_t)(best + T * c)];
                }
            }

        private:
            gpe_paths _ps = nullptr;
            HostPaths _host;
            int _D = 0, _P = 0, _S = 0;
            mean_fn _mean;

            void _swap(PathSet& o)
            {
                std::swap(_ps, o._ps);
                std::swap(_host, o._host);
                std::swap(_D, o._D);
                std::swap(_P, o._P);
                std::swap(_S, o._S);
                std::swap(_mean, o._mean);
            }
            void _release()
            {
                if (_ps)
                    gpe_paths_destroy(_ps);
                _ps = nullptr;
            }
            static void _check(int rc, const char* what)
            {
                if (rc < 0)
                    throw std::runtime_error(std::string("limbo_amd: ") + what + " failed: status " + std::to_string(rc));
            }
            void _stage(const std::vector<Eigen::VectorXd>& pts, std::vector<double>& Xq, std::vector<double>& mq) const
            {
                const int64_t T = pts.size();
                Xq.resize((size_t)(T * _D));
                mq.resize((size_t)(T * _P));
                for (int64_t t = 0; t < T; ++t) {
                    for (int d = 0; d < _D; ++d)
                        Xq[(size_t)(t * _D + d)] = pts[(size_t)t](d);
                    const Eigen::VectorXd mv = _mean(pts[(size_t)t]);
                    for (int p = 0; p < _P; ++p)
                        mq[(size_t)(t + T * p)] = mv(p);
                }
            }
            void _eval(const std::vector<Eigen::VectorXd>& pts, std::vector<Eigen::MatrixXd>* F, std::vector<Eigen::MatrixXd>* dF) const
            {
                const int64_t T = pts.size();
                const int nc = _S * _P;
                if (F)
                    F->assign((size_t)_S, Eigen::MatrixXd::Zero(T, _P));
                if (dF)
                    dF->assign((size_t)nc, Eigen::MatrixXd::Zero(T, _D));
                if (T == 0)
                    return;
                std::vector<double> Xq, mq, f(F ? (size_t)(T * nc) : 0), g(dF ? (size_t)(T * _D * nc) : 0);
                _stage(pts, Xq, mq);
                if (_ps)
                    _check(gpe_paths_eval(_ps, Xq.data(), T, mq.data(), F ? f.data() : nullptr, dF ? g.data() : nullptr), "gpe_paths_eval");
                else
                    _host.eval(Xq.data(), T, mq.data(), F ? f.data() : nullptr, dF ? g.data() : nullptr);
                for (int c = 0; c < nc; ++c) {
                    if (F)
                        for (int64_t t = 0; t < T; ++t)
                            (*F)[(size_t)(c % _S)](t, c / _S) = f[(size_t)(t + T * c)];
                    if (dF)
                        for (int d = 0; d < _D; ++d)
                            for (int64_t t = 0; t < T; ++t)
                                (*dF)[(size_t)c](t, d) = g[(size_t)(t + T * (d + (int64_t)_D * c))];
                }
            }
        };
    } // namespace pathwise
} // namespace limbo_amd
#endif
