// limbo/experimental/model/spgp.hpp — the sparse pseudo-input Gaussian process (SPGP / "FITC": Snelson & Ghahramani, Sparse
// Gaussian Processes using Pseudo-inputs, NIPS 2005) (contract: src/limbo/experimental/model/spgp.hpp:62-672).
//
// Same class shape and public surface as the reference; the model itself lives on the device behind include/gpe_sparse.h
// (limbo_amd/csrc/sparse.hpp, sparse.hip): L, V chunk by chunk, ep, the weighted Gram, Lm and bet of :394-406, the likelihood of
// :491, its gradient of :500-580 (include/gpe_sparse_grad.h), the predictions of :597-608 — O(N M^2) time, O(N + M^2) memory, N in the 10^5 .. 10^6.
//
// What differs, by decision:
//   - HyperParamsOptimizer defaults to opt::Rprop (the reference: NLOpt L-BFGS, which this tree does not have).
//   - optimize_hyperparams() initialises as :411-429 (a std::mt19937 instead of random_shuffle / srand(time)).  Value and analytic
//     gradient (:500-580) come from ONE gpe_sp_objective_grad per optimiser step (include/gpe_sparse_grad.h).  By default it fits
//     the D + 2 log-parameters b, c, sig with the pseudo-inputs HELD FIXED at their initial random subset.  Fitting the
//     pseudo-inputs is OPT-IN: with `BO_PARAM(bool, optimize_pseudo_inputs, true)` in Params::model_spgp (absent = false) and
//     pseudo-inputs that are not pinned, the parameter vector is the reference's (M + 1) D + 2 (:415), the pseudo-inputs in front,
//     packed column-major as HyperParams (:99-100) and the gradient dfw (:568) have them.  The start is written in that same
//     packing; the reference's :421 writes ROWS of the subset into the column-major vector, which scrambles the coordinates of
//     its initial pseudo-inputs (each still a mixture of data coordinates, none a data point) — not reproduced.
//     OUT OF SCOPE: a device-side optimiser loop (the optimiser stays on the host, one call per step) and a host path for small N
//     (every model, however small, is computed on the device).
//   - set_pseudo_samples / set_h_params / h_params / nlml (additions) pin a model: with pinned pseudo-inputs AND
//     hyper-parameters compute / add_sample / recompute do not optimise (the reference always does, :389-392), and predict does
//     not add the "+ sig" of an optimised model (:608) until optimize_hyperparams() has run.
//   - (n - m) / 2 of the likelihood is the real half (the reference divides integers, :491).
// Interface attribution: the template signature / policy shape of this header reproduces, by requirement (drop-in
// for user code), the public interface of resibots/limbo (Copyright Inria, 2015-; CeCILL-C licence, http://www.cecill.info),
// file named above.  The implementation behind the interface is this project's own.
#ifndef LIMBO_EXPERIMENTAL_MODEL_SPGP_HPP
#define LIMBO_EXPERIMENTAL_MODEL_SPGP_HPP
#include <algorithm>
#include <cassert>
#include <cmath>
#include <iostream>
#include <limits>
#include <numeric>
#include <random>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include <Eigen/Core>

#include <limbo/opt/optimizer.hpp>
#include <limbo/opt/rprop.hpp>
#include <limbo/tools/macros.hpp>
#include <limbo/tools/math.hpp>

#include "../../../../gpe_sparse.h"
#include "../../../../gpe_sparse_grad.h"

namespace limbo {
    namespace defaults {
        struct model_spgp {
            BO_PARAM(double, jitter, 0.000001);
            BO_PARAM(double, samples_percent, 10);
            BO_PARAM(int, min_m, 1);

            /// kernel parameters
            BO_PARAM(double, sig, 0.01);
            BO_PARAM(double, pred_kernel_sigma_sq, 0.5);
            BO_PARAM(double, pred_kernel_l, 0.5);
        };
    } // namespace defaults
} // namespace limbo

namespace limbo_amd {
    namespace detail {
        // Params::gpu::device() when the user's Params has one, 0 otherwise
        template <typename Params, typename = void>
        struct spgp_device {
            static int get() { return 0; }
        };
        template <typename Params>
        struct spgp_device<Params, decltype((void)Params::gpu::device())> {
            static int get() { return Params::gpu::device(); }
        };
        // Params::model_spgp::optimize_pseudo_inputs() when the user's Params has one, false otherwise
        template <typename Params, typename = void>
        struct spgp_fit_pseudo {
            static bool get() { return false; }
        };
        template <typename Params>
        struct spgp_fit_pseudo<Params, decltype((void)Params::model_spgp::optimize_pseudo_inputs())> {
            static bool get() { return Params::model_spgp::optimize_pseudo_inputs(); }
        };
    } // namespace detail
} // namespace limbo_amd

namespace limbo {
    namespace model {
        template <typename Params, typename KernelFunction, typename MeanFunction, class HyperParamsOptimizer = opt::Rprop<Params>>
        class SPGP {
        public:
            /// useful because the model might be created before knowing anything about the process
            SPGP() : _dim_in(-1), _dim_out(-1) {}

            /// useful because the model might be created before having samples
            SPGP(int dim_in, int dim_out) : _dim_in(dim_in), _dim_out(dim_out), _mean_function(dim_out), _kernel_function(dim_in) { _default_h_params(); }

            /// useful to construct without optimizing
            SPGP(const std::vector<Eigen::VectorXd>& samples, const std::vector<Eigen::VectorXd>& observations) { _init(_to_matrix(samples), _to_matrix(observations)); }

            ~SPGP()
            {
                if (_h)
                    gpe_sp_destroy(_h);
            }
            // the device model is rebuilt from the host copies on the next use
            SPGP(const SPGP& o) { _copy_from(o); }
            SPGP& operator=(const SPGP& o)
            {
                if (this != &o) {
                    if (_h)
                        gpe_sp_destroy(_h);
                    _h = nullptr;
                    _copy_from(o);
                }
                return *this;
            }

            /// execute the hyperparameters optimization
            void optimize_hyperparams()
            {
                _optimize_init = true;
                _optimize_hyperparams();
                _fit();
            }

            /// Compute the SPGP from samples and observations. This call needs to be explicit!
            void compute(const std::vector<Eigen::VectorXd>& samples, const std::vector<Eigen::VectorXd>& observations) { compute(_to_matrix(samples), _to_matrix(observations)); }
            void compute(const std::vector<Eigen::VectorXd>& samples, const Eigen::MatrixXd& observations) { compute(_to_matrix(samples), observations); }
            void compute(const Eigen::MatrixXd& samples, const Eigen::MatrixXd& observations)
            {
                assert(samples.rows() != 0);
                assert(observations.rows() != 0);
                assert(samples.rows() == observations.rows());
                _optimize_init = true;
                _init(samples, observations);
                _compute();
            }

            /// add sample and recompute the SPGP
            void add_sample(const Eigen::VectorXd& sample, const Eigen::VectorXd& observation)
            {
                if (_samples.rows() == 0) {
                    _dim_in = (int)sample.size();
                    _kernel_function = KernelFunction(_dim_in);
                    _dim_out = (int)observation.size();
                    _mean_function = MeanFunction(_dim_out);
                    if ((int)_b.size() != _dim_in)
                        _default_h_params();
                }
                else {
                    assert((int)sample.size() == _dim_in);
                    assert((int)observation.size() == _dim_out);
                }
                const int n = (int)_samples.rows();
                Eigen::MatrixXd S(n + 1, _dim_in), O(n + 1, _dim_out);
                for (int i = 0; i < n; ++i) {
                    for (int d = 0; d < _dim_in; ++d)
                        S(i, d) = _samples(i, d);
                    for (int p = 0; p < _dim_out; ++p)
                        O(i, p) = _observations(i, p);
                }
                for (int d = 0; d < _dim_in; ++d)
                    S(n, d) = sample(d);
                for (int p = 0; p < _dim_out; ++p)
                    O(n, p) = observation(p);
                _samples = S;
                _observations = O;
                _update_m();
                _compute_observations_zm();
                _data_dirty = true;
                _optimize_init = true;
                _compute();
            }

            /// return mu, sigma^2 of one point (spgp.hpp:193-197)
            std::tuple<Eigen::VectorXd, double> query(const Eigen::VectorXd& v) const
            {
                Eigen::MatrixXd xt(1, (int)v.size());
                for (int d = 0; d < (int)v.size(); ++d)
                    xt(0, d) = v(d);
                std::pair<Eigen::MatrixXd, Eigen::MatrixXd> r = predict(xt);
                Eigen::VectorXd mu(r.first.cols());
                for (int p = 0; p < (int)r.first.cols(); ++p)
                    mu(p) = r.first(0, p);
                return std::make_tuple(mu, r.second(0, 0));
            }

            /// return mu (T x dim_out), sigma^2 (T x 1). Predict a bunch of points (one per row).
            std::pair<Eigen::MatrixXd, Eigen::MatrixXd> predict(const Eigen::MatrixXd& xt) const { return _predict(xt, true, true); }

            Eigen::MatrixXd mu(const Eigen::MatrixXd& v) const { return _predict(_rows(v), true, false).first; }
            std::vector<Eigen::VectorXd> mu_mult(const Eigen::MatrixXd& v) const { return _to_vector(_predict(v, true, false).first); }
            double sigma(const Eigen::VectorXd& v) const
            {
                Eigen::MatrixXd xt(1, (int)v.size());
                for (int d = 0; d < (int)v.size(); ++d)
                    xt(0, d) = v(d);
                return _predict(xt, false, true).second(0, 0);
            }
            Eigen::VectorXd sigma_mult(const Eigen::MatrixXd& v) const
            {
                const Eigen::MatrixXd s = _predict(v, false, true).second;
                Eigen::VectorXd out(s.rows());
                for (int i = 0; i < (int)s.rows(); ++i)
                    out(i) = s(i, 0);
                return out;
            }

            int dim_in() const
            {
                assert(_dim_in != -1); // need to compute first !
                return _dim_in;
            }
            int dim_out() const
            {
                assert(_dim_out != -1); // need to compute first !
                return _dim_out;
            }

            const MeanFunction& mean_function() const { return _mean_function; }
            MeanFunction& mean_function() { return _mean_function; }

            /// return the maximum observation (only call this if the output of the GP is of dimension 1)
            Eigen::VectorXd max_observation() const
            {
                if (_observations.cols() > 1)
                    std::cout << "WARNING max_observation with multi dimensional observations doesn't make sense" << std::endl;
                return tools::make_vector(_observations.maxCoeff());
            }
            Eigen::VectorXd mean_observation() const { return _samples.rows() > 0 ? _obs_mean : Eigen::VectorXd::Zero(_dim_out); }

            int nb_samples() const { return (int)_samples.rows(); }
            int nb_pseudo_samples() const { return (int)_pseudo_samples.rows(); }

            ///  recomputes the SPGP
            void recompute(bool update_obs_mean = true)
            {
                (void)update_obs_mean;
                _optimize_init = true;
                _compute();
            }

            std::vector<Eigen::VectorXd> samples() const { return _to_vector(_samples); }
            std::vector<Eigen::VectorXd> pseudo_samples() const { return _to_vector(_pseudo_samples); }

            /// Addition: pin the pseudo-inputs (one per row)
            void set_pseudo_samples(const Eigen::MatrixXd& xb)
            {
                _pseudo_samples = xb;
                _pseudo_pinned = true;
                _pseudo_dirty = true;
                _fitted = false;
            }
            /// Addition: pin the hyper-parameters, in log-space as the reference's HyperParams (:94-101): b (dim_in), c, sig
            void set_h_params(const Eigen::VectorXd& log_b, double log_c, double log_sig)
            {
                _b = log_b;
                _c = log_c;
                _sig = log_sig;
                _hp_pinned = true;
                _fitted = false;
            }
            /// Addition: [log b_1 .. log b_D, log c, log sig]
            Eigen::VectorXd h_params() const
            {
                Eigen::VectorXd w(_b.size() + 2);
                for (int d = 0; d < (int)_b.size(); ++d)
                    w(d) = _b(d);
                w(_b.size()) = _c;
                w(_b.size() + 1) = _sig;
                return w;
            }
            /// Addition: the negative log marginal likelihood (:491) of the computed model, per output
            Eigen::VectorXd nlml() const
            {
                _require_fit();
                Eigen::VectorXd out(_dim_out);
                std::vector<double> v((size_t)_dim_out);
                _check(gpe_sp_nlml(_h, v.data()), "gpe_sp_nlml");
                for (int p = 0; p < _dim_out; ++p)
                    out(p) = v[(size_t)p];
                return out;
            }
            /// Addition: the status of the last device computation (0, or the 1-based first non-positive pivot: gpe_sparse.h)
            int status() const { return _status; }
            /// Addition: the seed of the random subset of :417-421
            void set_seed(unsigned long long s) { _rng.seed(s); }

        protected:
            size_t _m = 0;
            int _dim_in = -1;
            int _dim_out = -1;
            Eigen::MatrixXd _samples;
            Eigen::MatrixXd _observations;
            Eigen::MatrixXd _observations_zm;
            Eigen::VectorXd _obs_mean;
            MeanFunction _mean_function;
            KernelFunction _kernel_function;

            Eigen::MatrixXd _pseudo_samples;
            Eigen::VectorXd _b; // log b_d
            double _c = 0.0;    // log c (signal variance)
            double _sig = 0.0;  // log sig (noise variance)

            bool _optimize_init = true;
            bool _optimized = false;
            bool _pseudo_pinned = false, _hp_pinned = false;
            mutable bool _data_dirty = true, _pseudo_dirty = true, _fitted = false;
            mutable int _status = 0;
            mutable gpe_sp_handle _h = nullptr;
            HyperParamsOptimizer _hp_optimize;
            std::mt19937 _rng{std::random_device{}()};

            void _copy_from(const SPGP& o)
            {
                _m = o._m;
                _dim_in = o._dim_in;
                _dim_out = o._dim_out;
                _samples = o._samples;
                _observations = o._observations;
                _observations_zm = o._observations_zm;
                _obs_mean = o._obs_mean;
                _mean_function = o._mean_function;
                _kernel_function = o._kernel_function;
                _pseudo_samples = o._pseudo_samples;
                _b = o._b;
                _c = o._c;
                _sig = o._sig;
                _optimize_init = o._optimize_init;
                _optimized = o._optimized;
                _pseudo_pinned = o._pseudo_pinned;
                _hp_pinned = o._hp_pinned;
                _hp_optimize = o._hp_optimize;
                _rng = o._rng;
                _data_dirty = _pseudo_dirty = true;
                _fitted = false;
            }

            void _default_h_params()
            {
                // the reference keeps b, c, sig themselves (:112-114); here their logarithms
                _b = Eigen::VectorXd::Constant(_dim_in, std::log(Params::model_spgp::pred_kernel_l()));
                _c = std::log(Params::model_spgp::pred_kernel_sigma_sq());
                _sig = std::log(Params::model_spgp::sig());
            }

            void _init(const Eigen::MatrixXd& samples, const Eigen::MatrixXd& observations)
            {
                _samples = samples;
                _observations = observations;
                _dim_in = (int)_samples.cols();
                _dim_out = (int)_observations.cols();
                _mean_function = MeanFunction(_dim_out);
                _kernel_function = KernelFunction(_dim_in);
                if (!_hp_pinned || (int)_b.size() != _dim_in)
                    _default_h_params();
                _compute_observations_zm();
                _update_m();
                _data_dirty = true;
                _fitted = false;
                _optimize_init = true;
            }

            void _compute_observations_zm()
            {
                const int n = (int)_observations.rows();
                _obs_mean = Eigen::VectorXd::Zero(_dim_out);
                for (int p = 0; p < _dim_out; ++p) {
                    double s = 0.0;
                    for (int i = 0; i < n; ++i)
                        s += _observations(i, p);
                    _obs_mean(p) = s / n;
                }
                _observations_zm = Eigen::MatrixXd(n, _dim_out);
                Eigen::VectorXd x(_dim_in);
                for (int i = 0; i < n; ++i) {
                    for (int d = 0; d < _dim_in; ++d)
                        x(d) = _samples(i, d);
                    const Eigen::VectorXd mv = _mean_function(x, *this);
                    for (int p = 0; p < _dim_out; ++p)
                        _observations_zm(i, p) = _observations(i, p) - mv(p);
                }
            }

            void _update_m()
            {
                _m = (size_t)(Params::model_spgp::samples_percent() * _samples.rows() / 100);
                if (_m < (size_t)Params::model_spgp::min_m())
                    _m = (size_t)Params::model_spgp::min_m();
                if (_m > (size_t)_samples.rows())
                    _m = (size_t)_samples.rows();
            }

            /// spgp.hpp:389-407: optimise unless the model is pinned, then L, V, ep, Lm, bet on the device
            void _compute()
            {
                if (!(_pseudo_pinned && _hp_pinned))
                    _optimize_hyperparams();
                _fit();
            }

            void _check(int rc, const char* what) const
            {
                if (rc < 0)
                    throw std::runtime_error(std::string(what) + " failed with status " + std::to_string(rc) + ": " + (_h ? gpe_sp_last_error(_h) : ""));
            }

            // data and pseudo-inputs to the device where they changed
            void _upload() const
            {
                if (!_h)
                    _check(gpe_sp_create(limbo_amd::detail::spgp_device<Params>::get(), &_h), "gpe_sp_create");
                const int64_t n = _samples.rows();
                if (_data_dirty) {
                    std::vector<double> X((size_t)(n * _dim_in)), Y((size_t)(n * _dim_out));
                    for (int64_t i = 0; i < n; ++i)
                        for (int d = 0; d < _dim_in; ++d)
                            X[(size_t)(i * _dim_in + d)] = _samples(i, d);
                    for (int p = 0; p < _dim_out; ++p)
                        for (int64_t i = 0; i < n; ++i)
                            Y[(size_t)(i + p * n)] = _observations_zm(i, p);
                    _check(gpe_sp_set_data(_h, X.data(), n, _dim_in, Y.data(), _dim_out), "gpe_sp_set_data");
                    _data_dirty = false;
                    _pseudo_dirty = true;
                }
                if (_pseudo_dirty) {
                    const int64_t m = _pseudo_samples.rows();
                    std::vector<double> Xb((size_t)(m * _dim_in));
                    for (int64_t i = 0; i < m; ++i)
                        for (int d = 0; d < _dim_in; ++d)
                            Xb[(size_t)(i * _dim_in + d)] = _pseudo_samples(i, d);
                    _check(gpe_sp_set_pseudo(_h, Xb.data(), m), "gpe_sp_set_pseudo");
                    _pseudo_dirty = false;
                }
            }

            void _fit() const
            {
                _upload();
                std::vector<double> lb((size_t)_dim_in);
                for (int d = 0; d < _dim_in; ++d)
                    lb[(size_t)d] = _b(d);
                _check(gpe_sp_set_hparams(_h, lb.data(), _c, _sig, Params::model_spgp::jitter()), "gpe_sp_set_hparams");
                _status = gpe_sp_compute(_h);
                _check(_status, "gpe_sp_compute");
                _fitted = _status == 0;
            }

            void _require_fit() const
            {
                if (!_fitted)
                    _fit();
                if (!_fitted)
                    throw std::runtime_error("SPGP: the model could not be computed (non-positive pivot " + std::to_string(_status) + ")");
            }

            /// -nlml, summed over the outputs, at x = [the pseudo-inputs, column-major (only with nx = m dim_in > 0), log b, log c, log sig];
            /// with grad its gradient, from ONE gpe_sp_objective_grad (one `_likelihood(x, true)` of :446-451).  A failed factorisation is
            /// the worst value, with a zero gradient.
            double _objective(const Eigen::VectorXd& x, int nx, Eigen::VectorXd* grad = nullptr) const
            {
                const int m = (int)_pseudo_samples.rows();
                std::vector<double> lb((size_t)_dim_in), out((size_t)_dim_out), xb((size_t)nx), dxb((size_t)nx), dhp((size_t)_dim_in + 2);
                for (int j = 0; j < m && nx > 0; ++j)
                    for (int d = 0; d < _dim_in; ++d)
                        xb[(size_t)(j * _dim_in + d)] = x(j + d * m);
                for (int d = 0; d < _dim_in; ++d)
                    lb[(size_t)d] = x(nx + d);
                const double lc = x(nx + _dim_in), ls = x(nx + _dim_in + 1), jit = Params::model_spgp::jitter();
                int rc = 0;
                if (grad)
                    rc = gpe_sp_objective_grad(_h, nx > 0 ? xb.data() : nullptr, lb.data(), lc, ls, jit, out.data(), nx > 0 ? dxb.data() : nullptr,
                                               dhp.data());
                else {
                    if (nx > 0)
                        rc = gpe_sp_set_pseudo(_h, xb.data(), m);
                    if (rc == 0)
                        rc = gpe_sp_objective(_h, lb.data(), lc, ls, jit, out.data());
                }
                _fitted = false;
                if (nx > 0)
                    _pseudo_dirty = true; // (the device holds the last point evaluated, not _pseudo_samples)
                double s = 0.0;
                for (double v : out)
                    s += v;
                const bool ok = rc == 0 && std::isfinite(s);
                if (grad) {
                    *grad = Eigen::VectorXd(nx + _dim_in + 2);
                    for (int j = 0; j < m && nx > 0; ++j)
                        for (int d = 0; d < _dim_in; ++d)
                            (*grad)(j + d * m) = ok ? -dxb[(size_t)(j * _dim_in + d)] : 0.0;
                    for (int d = 0; d < _dim_in + 2; ++d)
                        (*grad)(nx + d) = ok ? -dhp[(size_t)d] : 0.0;
                }
                return ok ? -s : -std::numeric_limits<double>::max();
            }

            void _optimize_hyperparams()
            {
                const int n = (int)_samples.rows();
                if (_optimize_init) {
                    _update_m();
                    if (!_pseudo_pinned) {
                        // a random subset of the training inputs (:417-421)
                        std::vector<int> pos((size_t)n);
                        std::iota(pos.begin(), pos.end(), 0);
                        std::shuffle(pos.begin(), pos.end(), _rng);
                        _pseudo_samples = Eigen::MatrixXd((int)_m, _dim_in);
                        for (size_t i = 0; i < _m; ++i)
                            for (int d = 0; d < _dim_in; ++d)
                                _pseudo_samples((int)i, d) = _samples(pos[i], d);
                        _pseudo_dirty = true;
                    }
                    if (!_hp_pinned) {
                        // sensible values in log space (:423-426)
                        _b = Eigen::VectorXd(_dim_in);
                        for (int d = 0; d < _dim_in; ++d) {
                            double lo = _samples(0, d), hi = lo;
                            for (int i = 1; i < n; ++i) {
                                lo = std::min(lo, _samples(i, d));
                                hi = std::max(hi, _samples(i, d));
                            }
                            _b(d) = -2.0 * std::log(std::max((hi - lo) / 2.0, 1e-12));
                        }
                        double ms = 0.0;
                        for (int p = 0; p < _dim_out; ++p)
                            for (int i = 0; i < n; ++i)
                                ms += _observations_zm(i, p) * _observations_zm(i, p);
                        ms = std::max(ms / ((double)n * _dim_out), 1e-12);
                        _c = std::log(ms);
                        _sig = std::log(ms / 4.0);
                    }
                    _optimize_init = false;
                }
                _upload();
                // the parameter vector: [log b, log c, log sig], or — Params::model_spgp::optimize_pseudo_inputs(), pseudo-inputs not
                // pinned — the reference's (m + 1) dim_in + 2 (:415) with the pseudo-inputs in front, column-major
                const int m = (int)_pseudo_samples.rows();
                const int nx = (limbo_amd::detail::spgp_fit_pseudo<Params>::get() && !_pseudo_pinned) ? m * _dim_in : 0;
                auto objective = [&](const Eigen::VectorXd& x, bool g) -> opt::eval_t {
                    if (!g)
                        return opt::no_grad(this->_objective(x, nx));
                    Eigen::VectorXd grad;
                    const double f = this->_objective(x, nx, &grad);
                    return opt::eval_t{f, opt::optional_grad_t(grad)};
                };
                Eigen::VectorXd w0(nx + _dim_in + 2);
                for (int j = 0; j < m && nx > 0; ++j)
                    for (int d = 0; d < _dim_in; ++d)
                        w0(j + d * m) = _pseudo_samples(j, d);
                for (int d = 0; d < _dim_in; ++d)
                    w0(nx + d) = _b(d);
                w0(nx + _dim_in) = _c;
                w0(nx + _dim_in + 1) = _sig;
                const Eigen::VectorXd w = _hp_optimize(objective, w0, false);
                // (an optimiser that returns something worse than where it started is not followed)
                const Eigen::VectorXd& best = _objective(w, nx) >= _objective(w0, nx) ? w : w0;
                for (int j = 0; j < m && nx > 0; ++j)
                    for (int d = 0; d < _dim_in; ++d)
                        _pseudo_samples(j, d) = best(j + d * m);
                _b = Eigen::VectorXd(_dim_in);
                for (int d = 0; d < _dim_in; ++d)
                    _b(d) = best(nx + d);
                _c = best(nx + _dim_in);
                _sig = best(nx + _dim_in + 1);
                _optimized = true;
                _fitted = false;
            }

            std::pair<Eigen::MatrixXd, Eigen::MatrixXd> _predict(const Eigen::MatrixXd& xt, bool calc_mu = true, bool calc_s2 = true) const
            {
                const int64_t T = xt.rows();
                Eigen::MatrixXd mu(T, std::max(_dim_out, 0)), s2(T, 1);
                Eigen::VectorXd x(xt.cols());
                if (_samples.rows() == 0) { // :587-595: the prior
                    for (int64_t i = 0; i < T; ++i) {
                        for (int d = 0; d < (int)xt.cols(); ++d)
                            x(d) = xt(i, d);
                        if (calc_mu) {
                            const Eigen::VectorXd mv = _mean_function(x, *this);
                            for (int p = 0; p < _dim_out; ++p)
                                mu(i, p) = mv(p);
                        }
                        if (calc_s2)
                            s2(i, 0) = _kernel_function(x, x);
                    }
                    return {mu, s2};
                }
                _require_fit();
                std::vector<double> X((size_t)(T * _dim_in)), m((size_t)(T * _dim_out)), s((size_t)T);
                for (int64_t i = 0; i < T; ++i)
                    for (int d = 0; d < _dim_in; ++d)
                        X[(size_t)(i * _dim_in + d)] = xt(i, d);
                _check(gpe_sp_predict(_h, X.data(), T, calc_mu ? m.data() : nullptr, calc_s2 ? s.data() : nullptr), "gpe_sp_predict");
                const double add = _optimized ? std::exp(_sig) : 0.0; // :608
                for (int64_t i = 0; i < T; ++i) {
                    if (calc_mu) {
                        for (int d = 0; d < _dim_in; ++d)
                            x(d) = xt(i, d);
                        const Eigen::VectorXd mv = _mean_function(x, *this); // :602-604
                        for (int p = 0; p < _dim_out; ++p)
                            mu(i, p) = mv(p) + m[(size_t)(i + p * T)];
                    }
                    if (calc_s2)
                        s2(i, 0) = s[(size_t)i] + add;
                }
                return {mu, s2};
            }

            // a column vector is ONE point (the reference's mu(v) / sigma(v) take an Eigen::VectorXd where a row is expected)
            Eigen::MatrixXd _rows(const Eigen::MatrixXd& v) const
            {
                if (v.cols() == 1 && (int)v.rows() == _dim_in && _dim_in != 1) {
                    Eigen::MatrixXd r(1, _dim_in);
                    for (int d = 0; d < _dim_in; ++d)
                        r(0, d) = v(d, 0);
                    return r;
                }
                return v;
            }

            Eigen::MatrixXd _to_matrix(const std::vector<Eigen::VectorXd>& xs) const
            {
                Eigen::MatrixXd result((int)xs.size(), xs.empty() ? 0 : (int)xs[0].size());
                for (int i = 0; i < (int)result.rows(); ++i)
                    for (int d = 0; d < (int)result.cols(); ++d)
                        result(i, d) = xs[(size_t)i](d);
                return result;
            }
            std::vector<Eigen::VectorXd> _to_vector(const Eigen::MatrixXd& m) const
            {
                std::vector<Eigen::VectorXd> result((size_t)m.rows());
                for (size_t i = 0; i < result.size(); ++i) {
                    result[i] = Eigen::VectorXd(m.cols());
                    for (int d = 0; d < (int)m.cols(); ++d)
                        result[i](d) = m((int)i, d);
                }
                return result;
            }
        };
    } // namespace model
} // namespace limbo
#endif
