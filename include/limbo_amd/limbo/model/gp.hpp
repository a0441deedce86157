// limbo/model/gp.hpp — drop-in limbo::model::GP<Params, Kernel, Mean, HPOpt> whose linear algebra
// lives on an MI355X behind the C-ABI of include/gpe.h (libgpengine.so).
//
// Interface contract: src/limbo/model/gp.hpp:77-642 of resibots/limbo — same template
// parameters and defaults, same public members with the same meaning, same protected member
// names (subclasses and the reference's white-box tests touch _samples, _observations, _matrixL,
// _alpha ...: sparsified_gp.hpp:109-116, test_gp.cpp:1128-1155), same quirks:
//   * training K gets +noise+1e-8 on the diagonal (kernel.hpp:83); query()/sigma() add `noise` only
//   * sigma^2 is clamped to 0 when <= DBL_EPSILON before the noise is added (gp.hpp:621-623)
//   * log-lik: logdet and n log 2pi are NOT multiplied by dim_out (gp.hpp:274-279)
//   * no exception on a non-positive-definite K: NaNs propagate (gp.hpp:565); the pivot index the
//     device reports is kept in last_status()
// What is different is where the state lives: X, K/L, alpha, K^-1 are resident in HBM (one
// gpe_handle per GP, deep-copied by the copy constructor like the reference's value semantics);
// _matrixL/_alpha/_inv_kernel on the host are lazily filled mirrors.  The mean functor receives the
// GP itself and is evaluated on the host (gp.hpp:537-548); kernels without device code
// (limbo_amd::device_kernel<K>::kind == KIND_HOST_K) have their K and k* built by the functor on
// the host while factorisation and solves stay on the device.  There is no CPU fallback for the
// linear algebra: without libgpengine.so / a GPU, construction throws.
//
// Round 4: below Params::gpu::min_n_for_gpu() samples (default 256, limbo/model/gp/host_small.hpp) the factor and alpha live in
// the host matrices _matrixL / _alpha and compute(), add_sample(), recompute(), compute_log_lik() and the single-point query(),
// mu(), sigma() never touch the device: one core's O(n^2) call is cheaper than a launch plus a PCIe round trip (the BO inner
// loop of bayes_opt/boptimizer.hpp:148-161 on models of 10..200 samples).  Whatever has no host form — K^-1, the gradients,
// the LOO objectives, the batched hyper-parameter objectives — moves the model to the device for good (limbo_amd::Residency,
// gp/residency.hpp, keeps where it lives); a large
// query_batch() answers from a device copy of the host model that is refreshed when the host model has changed.
//
// Additions (not in the reference): query_batch() — the batched acquisition path of SURVEY.md
// §8 row a13/N1 — and last_status().
// Interface attribution: the template signature / policy shape of this header reproduces, by requirement (drop-in
// for user code), the public interface of resibots/limbo (Copyright Inria, 2015-; CeCILL-C licence, http://www.cecill.info),
// file named above.  The implementation behind the interface is this project's own.
#ifndef LIMBO_MODEL_GP_HPP
#define LIMBO_MODEL_GP_HPP

#include <algorithm>
#include <cassert>
#include <cfloat>
#include <cmath>
#include <iostream>
#include <limits>
#include <mutex>
#include <random>
#include <stdexcept>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include <Eigen/Core>

#include <limbo/kernel/matern_five_halves.hpp>
#include <limbo/kernel/squared_exp_ard.hpp>
#include <limbo/mean/constant.hpp>
#include <limbo/mean/data.hpp>
#include <limbo/model/gp/host_small.hpp>
#include <limbo/model/gp/replicas.hpp>
#include <limbo/model/gp/residency.hpp>
#include <limbo/model/gp/query_grad.hpp>
#include <limbo/model/gp/pathwise.hpp>
#include <limbo/model/gp/kg.hpp>
#include <limbo/model/gp/ehvi.hpp>
#include <limbo/model/gp/ehvi3.hpp>
#include <limbo/model/gp/cei.hpp>
#include <limbo/model/gp/mes.hpp>
#include <limbo/model/gp/nei.hpp>
#include <limbo/model/gp/kernel_lf_opt.hpp>
#include <limbo/model/gp/no_lf_opt.hpp>
#include <limbo/tools/math.hpp>
#include <limbo/tools/parallel.hpp>

#include "../../../gpe.h"
#include "../../../gpe_joint.h"
#include "../../../gpe_append.h"
#include "../../../gpe_remove.h"
#include "../../../gpe_query_grad.h"
#include "../../../gpe_batch_select.h"
#include "../../../gpe_kg.h"
#include "../../../gpe_ehvi.h"
#include "../../../gpe_ehvi3.h"
#include "../../../gpe_cei.h"
#include "../../../gpe_mes.h"
#include "../../../gpe_nei.h"

namespace limbo {
    namespace model {
        template <typename Params, typename KernelFunction = kernel::MaternFiveHalves<Params>, typename MeanFunction = mean::Data<Params>, typename HyperParamsOptimizer = gp::NoLFOpt<Params>>
        class GP {
        public:
            GP() : _dim_in(-1), _dim_out(-1), _log_lik(0), _log_loo_cv(0), _inv_kernel_updated(false), _eng(limbo_amd::home_device<Params>()) {}

            GP(int dim_in, int dim_out)
                : _dim_in(dim_in), _dim_out(dim_out), _kernel_function(dim_in), _mean_function(dim_out), _log_lik(0), _log_loo_cv(0), _inv_kernel_updated(false), _eng(limbo_amd::home_device<Params>()) {}

            /// value semantics as in the reference: the device state is deep-copied (gpe_clone)
            GP(const GP& o) : GP(o, o._eng.device()) {}

            /// the same onto another device of the node (addition: how the parallel policies spread independent GPs)
            GP(const GP& o, int device)
                : _dim_in(o._dim_in), _dim_out(o._dim_out), _kernel_function(o._kernel_function), _mean_function(o._mean_function), _samples(o._samples), _observations(o._observations), _mean_vector(o._mean_vector), _obs_mean(o._obs_mean), _alpha(o._alpha), _mean_observation(o._mean_observation), _kernel(o._kernel), _inv_kernel(o._inv_kernel), _matrixL(o._matrixL), _log_lik(o._log_lik), _log_loo_cv(o._log_loo_cv), _inv_kernel_updated(o._inv_kernel_updated), _hp_optimize(o._hp_optimize), _eng(o._eng, device), _status(o._status), _res(o._res.for_copy()) {}

            /// device this GP lives on / move it (additions)
            int device() const { return _eng.device(); }
            void set_device(int device)
            {
                _eng.set_device(device);
                release_query_replicas(); // (they were dealt around the old home)
            }

            GP& operator=(const GP& o)
            {
                if (this != &o) {
                    GP tmp(o);
                    _swap(tmp);
                }
                return *this;
            }

            /// gp.hpp:88-116
            void compute(const std::vector<Eigen::VectorXd>& samples, const std::vector<Eigen::VectorXd>& observations, bool compute_kernel = true)
            {
                assert(samples.size() != 0);
                assert(observations.size() != 0);
                assert(samples.size() == observations.size());

                _adopt_dims((int)samples[0].size(), (int)observations[0].size());
                _samples = samples;
                _observations.resize(observations.size(), _dim_out);
                for (int i = 0; i < (int)_observations.rows(); ++i)
                    for (int p = 0; p < _dim_out; ++p)
                        _observations(i, p) = observations[i](p);
                _update_mean_observation();
                this->_compute_obs_mean();
                _res.return_to_full_path();
                if (compute_kernel)
                    this->_compute_full_kernel();
            }

            /// gp.hpp:119-122
            void optimize_hyperparams() { _hp_optimize(*this); }

            /// gp.hpp:126-152 — one row appended to L on the device (capacity-doubling buffers, no
            /// O(n^2) reallocation per sample)
            void add_sample(const Eigen::VectorXd& sample, const Eigen::VectorXd& observation)
            {
                if (_samples.empty())
                    _adopt_dims((int)sample.size(), (int)observation.size());
                else {
                    assert((int)sample.size() == _dim_in);
                    assert((int)observation.size() == _dim_out);
                }
                _samples.push_back(sample);
                _observations.conservativeResize(_observations.rows() + 1, _dim_out);
                for (int p = 0; p < _dim_out; ++p)
                    _observations(_observations.rows() - 1, p) = observation(p);
                _update_mean_observation();
                this->_compute_obs_mean();
                this->_compute_incremental_kernel();
            }

            /// A batch of samples in one blocked update (include/gpe_append.h): what add_sample() for each of them in order leaves,
            /// to rounding — the q observations of a batch-acquisition round (acqui/thompson.hpp) go in with ONE mean / obs_mean
            /// update, one append of q rows to L and one alpha solve.  The shape checks are add_sample's (gp.hpp:126-152).
            void add_samples(const std::vector<Eigen::VectorXd>& samples, const std::vector<Eigen::VectorXd>& observations)
            {
                assert(samples.size() == observations.size());
                const int64_t q = (int64_t)samples.size();
                if (q == 0)
                    return;
                if (_samples.empty())
                    _adopt_dims((int)samples[0].size(), (int)observations[0].size());
                for (int64_t i = 0; i < q; ++i) {
                    assert((int)samples[i].size() == _dim_in);
                    assert((int)observations[i].size() == _dim_out);
                }
                const int64_t n0 = (int64_t)_samples.size();
                _samples.insert(_samples.end(), samples.begin(), samples.end());
                _observations.conservativeResize(n0 + q, _dim_out);
                for (int64_t i = 0; i < q; ++i)
                    for (int p = 0; p < _dim_out; ++p)
                        _observations(n0 + i, p) = observations[i](p);
                _update_mean_observation();
                this->_compute_obs_mean();
                this->_compute_incremental_block(n0);
            }

            /// Addition (include/gpe_remove.h): the samples at `indices` (any order, distinct) leave the model; what compute() on the
            /// remaining samples in their order leaves, to rounding — by an update of the factor that costs far less than the
            /// factorisation.  The mean functor sees the new data.  Removing every sample leaves the empty model of the same
            /// dimensions: query() then answers the prior, as after construction.
            void remove_samples(const std::vector<size_t>& indices)
            {
                if (indices.empty())
                    return;
                std::vector<int64_t> R(indices.begin(), indices.end());
                std::sort(R.begin(), R.end());
                const int64_t n0 = (int64_t)_samples.size(), q = (int64_t)R.size();
                assert(R.back() < n0 && std::adjacent_find(R.begin(), R.end()) == R.end());
                if (q >= n0) {
                    _samples.clear();
                    _observations.resize(0, _dim_out);
                    _update_mean_observation();
                    _mean_vector.resize(0, _dim_out);
                    _obs_mean.resize(0, _dim_out);
                    _alpha.resize(0, _dim_out);
                    _matrixL.resize(0, 0);
                    _emptied();
                    release_query_replicas();
                    return;
                }
                std::vector<Eigen::VectorXd> kept;
                kept.reserve((size_t)(n0 - q));
                Eigen::MatrixXd obs(n0 - q, _dim_out);
                for (int64_t i = 0, k = 0; i < n0; ++i) {
                    if (k < q && R[(size_t)k] == i) {
                        ++k;
                        continue;
                    }
                    for (int p = 0; p < _dim_out; ++p)
                        obs((int)kept.size(), p) = _observations(i, p);
                    kept.push_back(_samples[(size_t)i]);
                }
                _samples.swap(kept);
                _observations = obs;
                _update_mean_observation();
                this->_compute_obs_mean();
                this->_compute_removed(R, n0);
            }

            /// gp.hpp:159-167
            std::tuple<Eigen::VectorXd, double> query(const Eigen::VectorXd& v) const
            {
                if (_samples.size() == 0)
                    return std::make_tuple(_mean_function(v, *this), _kernel_function(v, v) + _kernel_function.noise());
                Eigen::VectorXd kta;
                double var;
                _query_one(v, &kta, &var);
                return std::make_tuple(_finish_mu(v, kta), _finish_sigma(var) + _kernel_function.noise());
            }

            /// gp.hpp:174-179
            Eigen::VectorXd mu(const Eigen::VectorXd& v) const
            {
                if (_samples.size() == 0)
                    return _mean_function(v, *this);
                Eigen::VectorXd kta;
                _query_one(v, &kta, nullptr);
                return _finish_mu(v, kta);
            }

            /// gp.hpp:186-191
            double sigma(const Eigen::VectorXd& v) const
            {
                if (_samples.size() == 0)
                    return _kernel_function(v, v) + _kernel_function.noise();
                double var;
                _query_one(v, nullptr, &var);
                return _finish_sigma(var) + _kernel_function.noise();
            }

            /// Batched query (not in the reference, which loops over query()):
            /// mu is M x dim_out, sigma_sq has M entries; row m equals query(points[m]).
            void query_batch(const std::vector<Eigen::VectorXd>& points, Eigen::MatrixXd& mu_out, Eigen::VectorXd& sigma_sq) const
            {
                const int64_t M = points.size();
                mu_out.resize(M, _dim_out);
                sigma_sq.resize(M);
                if (M == 0)
                    return;
                if (_samples.size() == 0) {
                    for (int64_t m = 0; m < M; ++m) {
                        Eigen::VectorXd mv = _mean_function(points[m], *this);
                        for (int p = 0; p < _dim_out; ++p)
                            mu_out(m, p) = mv(p);
                        sigma_sq(m) = _kernel_function(points[m], points[m]) + _kernel_function.noise();
                    }
                    return;
                }
                std::vector<double> kta((size_t)(M * _dim_out)), var((size_t)M);
                if (_res.on_host() && M * (int64_t)_samples.size() < (int64_t)limbo_amd::host_batch_crossover())
                    for (int64_t m = 0; m < M; ++m) { // a handful of points on a small model: still cheaper here
                        _host_query(points[m], &kta[(size_t)m], M, &var[(size_t)m]);
                    }
                else
                    _query_many(points, kta.data(), var.data());
                for (int64_t m = 0; m < M; ++m) {
                    Eigen::VectorXd mv = _mean_function(points[m], *this);
                    for (int p = 0; p < _dim_out; ++p)
                        mu_out(m, p) = kta[(size_t)(m + M * p)] + mv(p);
                    sigma_sq(m) = _finish_sigma(var[(size_t)m]) + _kernel_function.noise();
                }
            }

            /// Addition (include/gpe_query_grad.h): query_batch() together with the posterior's GRADIENT in the point — what a
            /// gradient optimiser of an acquisition function consumes.  mu and sigma_sq are exactly query_batch()'s (mean functor
            /// added, clamp, + noise); dmu[m] is dim_out x dim_in, dmu[m](p, d) = d mu_p / d v_d at points[m]; dsigma_sq is
            /// M x dim_in, its row m zero where _finish_sigma clamped the variance.  The mean functor's OWN derivative is not
            /// included: exact for mean::NullFunction, mean::Constant and mean::Data, whose value does not depend on the point.
            /// Runs on the model's home device (the dealing of large query_batch() calls over devices does not apply); no samples:
            /// zeros; a host-resident model with M n below the batch crossover: on the host from matrixL() and
            /// limbo_amd::query_grad::dk_dv; kernels without device code: std::logic_error.
            void query_grad_batch(const std::vector<Eigen::VectorXd>& points, Eigen::MatrixXd& mu_out, Eigen::VectorXd& sigma_sq,
                std::vector<Eigen::MatrixXd>& dmu, Eigen::MatrixXd& dsigma_sq) const
            {
                const int64_t M = points.size(), n = _samples.size();
                const int D = _dim_in, P = _dim_out;
                mu_out.resize(M, P);
                sigma_sq.resize(M);
                dmu.assign((size_t)M, Eigen::MatrixXd::Zero(P, D));
                dsigma_sq = Eigen::MatrixXd::Zero(M, D);
                if (M == 0)
                    return;
                if (n == 0) {
                    query_batch(points, mu_out, sigma_sq);
                    return;
                }
                constexpr int kind = limbo_amd::device_kernel<KernelFunction>::kind;
                if (kind == limbo_amd::KIND_HOST_K)
                    throw std::logic_error("limbo_amd: query_grad_batch(): this kernel has no device code, hence no derivative in the query point");
                std::vector<double> kta((size_t)(M * P)), var((size_t)M), dkta((size_t)(M * D * P)), dvar((size_t)(M * D));
                if (_res.on_host() && M * n < (int64_t)limbo_amd::host_batch_crossover())
                    _host_query_grad(points, kta.data(), var.data(), dkta.data(), dvar.data());
                else {
                    const std::vector<double> Xq = _joint_points(points);
                    _eng.check(gpe_query_batch_grad(_eng.get(), Xq.data(), M, kta.data(), var.data(), dkta.data(), dvar.data()), "gpe_query_batch_grad");
                }
                for (int64_t m = 0; m < M; ++m) {
                    Eigen::VectorXd mv = _mean_function(points[m], *this);
                    for (int p = 0; p < P; ++p) {
                        mu_out(m, p) = kta[(size_t)(m + M * p)] + mv(p);
                        for (int d = 0; d < D; ++d)
                            dmu[(size_t)m](p, d) = dkta[(size_t)(m + M * (d + (int64_t)D * p))];
                    }
                    const double s2 = _finish_sigma(var[(size_t)m]);
                    sigma_sq(m) = s2 + _kernel_function.noise();
                    if (s2 != 0)
                        for (int d = 0; d < D; ++d)
                            dsigma_sq(m, d) = dvar[(size_t)(m + M * d)];
                }
            }

            /// Addition (include/gpe_joint.h): the JOINT posterior of a batch — mu (M x dim_out, the mean functor added, as
            /// query_batch) and the full predictive covariance cov (M x M, symmetric; one matrix serves all outputs):
            /// cov(a, b) = k(v_a, v_b) - (L^-1 k_a).(L^-1 k_b) + jitter [a == b], the kernel WITHOUT noise and without the clamp of
            /// gp.hpp:621-623, so cov(m, m) == sigma(points[m]) - noise where that is above the clamp.  Runs on the model's home
            /// device (cov couples the points: the dealing of large query_batch() calls over devices does not apply); no samples:
            /// the prior; a host-resident model below the batch crossover, and kernels without device code: on the host from
            /// matrixL() (O(M n^2 + M^2 n) scalar work — slow for large models).
            void query_joint(const std::vector<Eigen::VectorXd>& points, Eigen::MatrixXd& mu_out, Eigen::MatrixXd& cov, double jitter = 0) const
            {
                const int64_t M = points.size();
                mu_out.resize(M, _dim_out);
                cov.resize(M, M);
                if (M == 0)
                    return;
                std::vector<double> kta((size_t)(M * _dim_out), 0.0);
                if (_joint_on_host(M))
                    _host_joint(points, kta.data(), cov.data(), jitter);
                else {
                    const std::vector<double> Xq = _joint_points(points);
                    _eng.check(gpe_joint_query(_eng.get(), Xq.data(), M, jitter, kta.data(), cov.data(), M), "gpe_joint_query");
                }
                for (int64_t m = 0; m < M; ++m) {
                    Eigen::VectorXd mv = _mean_function(points[m], *this);
                    for (int p = 0; p < _dim_out; ++p)
                        mu_out(m, p) = kta[(size_t)(m + M * p)] + mv(p);
                }
            }

            /// Addition: n_draws function draws from the joint posterior at `points`, one M x dim_out matrix per draw:
            /// F_s = m(V) + k(V, X) alpha + chol(cov + jitter I) Z_s with the standard normals Z (M x n_draws x dim_out, point
            /// fastest, then draw) supplied by the caller: a deterministic function of (model, points, jitter, Z).  jitter = the
            /// kernel's noise gives draws of noisy observations, a small value draws of f.  Throws std::runtime_error when
            /// cov + jitter I is not positive definite.
            std::vector<Eigen::MatrixXd> sample(const std::vector<Eigen::VectorXd>& points, const std::vector<double>& Z, int n_draws, double jitter) const
            {
                const int64_t M = points.size();
                std::vector<double> F((size_t)(M * n_draws * _dim_out));
                _draws(points, Z, n_draws, jitter, F.data(), nullptr, nullptr);
                std::vector<Eigen::MatrixXd> out;
                for (int s = 0; s < n_draws; ++s) {
                    Eigen::MatrixXd f(M, _dim_out);
                    for (int p = 0; p < _dim_out; ++p)
                        for (int64_t m = 0; m < M; ++m)
                            f(m, p) = F[(size_t)(m + M * (s + (int64_t)n_draws * p))];
                    out.push_back(f);
                }
                return out;
            }
            /// ... with Z from std::mt19937_64(seed) through std::normal_distribution, in the order of Z's layout
            std::vector<Eigen::MatrixXd> sample(const std::vector<Eigen::VectorXd>& points, int n_draws, uint64_t seed, double jitter) const
            {
                return sample(points, standard_normals((size_t)points.size() * (size_t)n_draws * (size_t)_dim_out, seed), n_draws, jitter);
            }
            static std::vector<double> standard_normals(size_t n, uint64_t seed)
            {
                std::mt19937_64 gen(seed);
                std::normal_distribution<double> nd(0.0, 1.0);
                std::vector<double> z(n);
                for (double& v : z)
                    v = nd(gen);
                return z;
            }
            /// Addition: per draw s and output p the index of the point with the largest value (the lowest one on exact ties) and
            /// that value, argmax[s + n_draws p] — on the device the draws themselves never leave it (acqui/thompson.hpp)
            void sample_argmax(const std::vector<Eigen::VectorXd>& points, const std::vector<double>& Z, int n_draws, double jitter,
                std::vector<int64_t>& argmax, std::vector<double>& fmax) const
            {
                argmax.assign((size_t)(n_draws * _dim_out), 0);
                fmax.assign((size_t)(n_draws * _dim_out), 0.0);
                _draws(points, Z, n_draws, jitter, nullptr, argmax.data(), fmax.data());
            }

            /// Addition (include/gpe_batch_select.h): q greedy picks among `points` from ONE model state — take the maximiser of
            /// the score, condition the posterior variance on a hallucinated observation of noise obs_noise there (the mean stays),
            /// take the next (GP-BUCB, kriging believer, max-variance design; acqui/batch_select.hpp wraps the first two).
            /// rule: GPE_SELECT_UCB (param = beta), GPE_SELECT_EI (param = f+ + jitter) or GPE_SELECT_VAR.  mu: one COMPLETE value
            /// per point (mean functor and aggregator applied by the caller), or empty: k(X, v)^T alpha of output 0 with no mean
            /// functor.  var_add is added to the clamped variance in the score (the kernel's noise for what query() reports).
            /// idx / score: the pick and its score per round.  Returns 0, or t + 1 when round t's pivot is not positive: idx and
            /// score then end with round t.  On the model's home device; no samples (the prior), a host-resident model below the
            /// batch crossover and kernels without device code: on the host from the M x M covariance of query_joint.
            int select_batch(const std::vector<Eigen::VectorXd>& points, int q, int rule, double param, const std::vector<double>& mu,
                double var_add, double obs_noise, bool distinct, std::vector<int64_t>& idx, std::vector<double>& score) const
            {
                const int64_t M = points.size();
                if (q < 0 || q > GPE_SELECT_MAX_ROUNDS || rule < GPE_SELECT_UCB || rule > GPE_SELECT_VAR || !std::isfinite(param)
                    || (rule == GPE_SELECT_UCB && param < 0) || !(var_add >= 0) || !std::isfinite(var_add) || !(obs_noise >= 0)
                    || !std::isfinite(obs_noise) || (distinct && q > M && M > 0) || (!mu.empty() && (int64_t)mu.size() != M))
                    throw std::invalid_argument("limbo_amd: select_batch(): bad argument (include/gpe_batch_select.h)");
                idx.assign((size_t)q, -1);
                score.assign((size_t)q, 0.0);
                if (M == 0 || q == 0) {
                    idx.clear();
                    score.clear();
                    return 0;
                }
                int rc = 0;
                if (_joint_on_host(M)) {
                    std::vector<double> kta((size_t)(M * _dim_out)), cov((size_t)(M * M)), var((size_t)M), W((size_t)(M * q));
                    _host_joint(points, kta.data(), cov.data(), 0.0);
                    rc = limbo_amd::host_small::select_greedy(cov.data(), M, M, mu.empty() ? kta.data() : mu.data(), q, rule, param, var_add,
                        obs_noise, distinct, idx.data(), score.data(), var.data(), W.data());
                }
                else {
                    const std::vector<double> Xq = _joint_points(points);
                    rc = _eng.check(gpe_select_batch(_eng.get(), Xq.data(), M, q, rule, param, mu.empty() ? nullptr : mu.data(), var_add, obs_noise,
                                        distinct ? 1 : 0, idx.data(), score.data(), nullptr, nullptr, 0),
                        "gpe_select_batch");
                }
                if (rc > 0) {
                    idx.resize((size_t)rc);
                    score.resize((size_t)rc);
                }
                return rc;
            }

            /// Addition (include/gpe_kg.h, model/gp/kg.hpp): the knowledge gradient with correlated beliefs of every candidate over
            /// a finite set of alternatives — the expected rise of the best posterior mean over the alternatives after ONE
            /// observation of noise obs_noise at the candidate; with_self: the candidate counts among the alternatives.  mu_a / mu_c:
            /// one COMPLETE mean per alternative / candidate (mean functor and aggregator applied by the caller), or empty:
            /// k(X, v)^T alpha of output 0 with no mean functor (a constant mean moves nothing: the means enter as differences).
            /// The model is not changed.  On the model's home device; no samples (the prior), a host-resident model below the
            /// batch crossover and kernels without device code: on the host from the covariance of query_joint.
            void knowledge_gradient(const std::vector<Eigen::VectorXd>& alternatives, const std::vector<Eigen::VectorXd>& candidates,
                const std::vector<double>& mu_a, const std::vector<double>& mu_c, double obs_noise, bool with_self, std::vector<double>& kg) const
            {
                const int64_t A = alternatives.size(), M = candidates.size();
                if (A < 1 || A > GPE_KG_MAX_ALTERNATIVES || !(obs_noise >= 0) || !std::isfinite(obs_noise)
                    || (!mu_a.empty() && (int64_t)mu_a.size() != A) || (!mu_c.empty() && (int64_t)mu_c.size() != M))
                    throw std::invalid_argument("limbo_amd: knowledge_gradient(): bad argument (include/gpe_kg.h)");
                kg.assign((size_t)M, 0.0);
                if (M == 0)
                    return;
                if (_joint_on_host(A + M)) {
                    std::vector<Eigen::VectorXd> pts(alternatives);
                    pts.insert(pts.end(), candidates.begin(), candidates.end());
                    const int64_t T = A + M;
                    std::vector<double> kta((size_t)(T * _dim_out)), cov((size_t)(T * T));
                    _host_joint(pts, kta.data(), cov.data(), 0.0);
                    if (!mu_a.empty())
                        std::copy(mu_a.begin(), mu_a.end(), kta.begin());
                    if (!mu_c.empty())
                        std::copy(mu_c.begin(), mu_c.end(), kta.begin() + A);
                    limbo_amd::kg_host::from_joint(cov.data(), kta.data(), A, M, obs_noise, with_self, kg.data());
                }
                else {
                    const std::vector<double> Xa = _joint_points(alternatives), Xc = _joint_points(candidates);
                    _eng.check(gpe_kg_batch(_eng.get(), Xa.data(), A, mu_a.empty() ? nullptr : mu_a.data(), Xc.data(), M,
                                   mu_c.empty() ? nullptr : mu_c.data(), obs_noise, with_self ? 1 : 0, kg.data(), nullptr, nullptr, 0),
                        "gpe_kg_batch");
                }
            }
            /// ... with k(X, v)^T alpha of output 0 as the means and the kernel's noise as the observation's
            void knowledge_gradient(const std::vector<Eigen::VectorXd>& alternatives, const std::vector<Eigen::VectorXd>& candidates, bool with_self,
                std::vector<double>& kg) const
            {
                knowledge_gradient(alternatives, candidates, {}, {}, _kernel_function.noise(), with_self, kg);
            }

            /// Addition (include/gpe_ehvi.h, model/gp/ehvi.hpp): the exact expected hypervolume improvement of every candidate
            /// under TWO outputs of this model (out1 != out2, both maximised; they share sigma: limbo's GP with dim_out = 2) over
            /// a prepared front (row-major n x 2: ascending in output out1, descending in out2, all above ref; limbo_amd::
            /// pareto_front2 makes one).  The means are k^T alpha plus the mean functor; sigma^2 is the clamped variance of the
            /// LATENT function, or, observation == true, with the kernel's noise added (what query() reports).  Unlike the
            /// reference's experimental/acqui/ehvi.hpp:76 the strip sum is given a standard deviation, not sigma(v).  partials
            /// (may be null): M x 4 column-major, d/d mu1, d/d s1, d/d mu2, d/d s2.  The model is not changed.  On the model's
            /// home device; no samples (the prior), a host-resident model below the batch crossover and kernels without device
            /// code: query_batch() and the host strip sum of the same definition.
            void expected_hypervolume_improvement(const std::vector<Eigen::VectorXd>& candidates, const std::vector<double>& front,
                const double* ref, int out1, int out2, bool observation, std::vector<double>& ehvi, std::vector<double>* partials = nullptr) const
            {
                const int64_t M = candidates.size(), n = (int64_t)front.size() / 2;
                const std::vector<int> outs{out1, out2};
                if (front.size() % 2 != 0 || !_outputs_ok(outs) || !ref || n > GPE_EHVI_MAX_FRONT
                    || gpe_ehvi2_values(nullptr, front.data(), n, ref, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr) != GPE_OK)
                    throw std::invalid_argument("limbo_amd: expected_hypervolume_improvement(): bad argument (include/gpe_ehvi.h)");
                _zeroed(M, ehvi, partials, 4, nullptr, 0);
                if (M == 0)
                    return;
                if (_joint_on_host(M)) {
                    std::vector<double> mu, sd;
                    _beliefs_of(candidates, outs, observation, mu, sd);
                    limbo_amd::ehvi_host::strip_sums(front.data(), n, ref, mu.data(), sd.data(), mu.data() + M, sd.data() + M, M, ehvi.data(),
                        _data(partials));
                    return;
                }
                const std::vector<double> Xc = _joint_points(candidates), add = _mean_add(candidates, outs);
                _eng.check(gpe_ehvi2_batch(_eng.get(), out1, out2, Xc.data(), M, add.data(), observation ? _kernel_function.noise() : 0.0, front.data(), n,
                               ref, ehvi.data(), _data(partials), nullptr, nullptr),
                    "gpe_ehvi2_batch");
            }
            /// Does this model hold an engine handle a caller's own beliefs can be scored through (ehvi2_values)?
            bool has_engine() const
            {
                return !_res.on_host() && _eng.peek() != nullptr && limbo_amd::device_kernel<KernelFunction>::kind != limbo_amd::KIND_HOST_K;
            }
            /// gpe_ehvi2_values through this model's engine handle (has_engine()): the strip sums of beliefs the caller computed
            void ehvi2_values(const std::vector<double>& front, const double* ref, const std::vector<double>& mu1, const std::vector<double>& s1,
                const std::vector<double>& mu2, const std::vector<double>& s2, std::vector<double>& ehvi, std::vector<double>* partials = nullptr) const
            {
                const int64_t M = mu1.size();
                _zeroed(M, ehvi, partials, 4, nullptr, 0);
                _eng.check(gpe_ehvi2_values(_eng.get(), front.data(), (int64_t)front.size() / 2, ref, mu1.data(), s1.data(), mu2.data(), s2.data(), M,
                               ehvi.data(), _data(partials)),
                    "gpe_ehvi2_values");
            }

            /// Addition (include/gpe_ehvi3.h, model/gp/ehvi3.hpp): the exact expected hypervolume improvement of every candidate
            /// under THREE outputs of this model (outs: pairwise distinct, all maximised; they share sigma: limbo's GP with
            /// dim_out = 3) over a prepared front (row-major n x 3: descending in the third of them, none dominated, all above
            /// ref; limbo_amd::pareto_front3 makes one).  Means, sigma and `observation` as for two objectives above.  partials
            /// (may be null): M x 6 column-major, d/d mu1, d/d s1, d/d mu2, d/d s2, d/d mu3, d/d s3.  The model is not changed.
            /// On the model's home device; no samples (the prior), a host-resident model below the batch crossover and kernels
            /// without device code: query_batch() and the host box sums of the same definition.
            void expected_hypervolume_improvement3(const std::vector<Eigen::VectorXd>& candidates, const std::vector<double>& front,
                const double* ref, const std::vector<int>& outs, bool observation, std::vector<double>& ehvi,
                std::vector<double>* partials = nullptr) const
            {
                const int64_t M = candidates.size(), n = (int64_t)front.size() / 3;
                if (front.size() % 3 != 0 || outs.size() != 3 || !_outputs_ok(outs) || !ref
                    || gpe_ehvi3_values(nullptr, front.data(), n, ref, nullptr, nullptr, 0, nullptr, nullptr) != GPE_OK)
                    throw std::invalid_argument("limbo_amd: expected_hypervolume_improvement3(): bad argument (include/gpe_ehvi3.h)");
                _zeroed(M, ehvi, partials, 6, nullptr, 0);
                if (M == 0)
                    return;
                if (_joint_on_host(M)) {
                    std::vector<double> mu, sd;
                    _beliefs_of(candidates, outs, observation, mu, sd);
                    limbo_amd::ehvi3_host::Tables t;
                    limbo_amd::ehvi3_host::tables(front.data(), n, ref, partials != nullptr, t);
                    limbo_amd::ehvi3_host::box_sums(t, mu.data(), sd.data(), M, ehvi.data(), _data(partials));
                    return;
                }
                const std::vector<double> Xc = _joint_points(candidates), add = _mean_add(candidates, outs);
                _eng.check(gpe_ehvi3_batch(_eng.get(), outs.data(), Xc.data(), M, add.data(), observation ? _kernel_function.noise() : 0.0,
                               front.data(), n, ref, ehvi.data(), _data(partials), nullptr, nullptr),
                    "gpe_ehvi3_batch");
            }
            /// gpe_ehvi3_values through this model's engine handle (has_engine()): the box sums of beliefs the caller computed, mu
            /// and s M x 3 column-major
            void ehvi3_values(const std::vector<double>& front, const double* ref, const std::vector<double>& mu, const std::vector<double>& s,
                std::vector<double>& ehvi, std::vector<double>* partials = nullptr) const
            {
                const int64_t M = (int64_t)mu.size() / 3;
                _zeroed(M, ehvi, partials, 6, nullptr, 0);
                _eng.check(gpe_ehvi3_values(_eng.get(), front.data(), (int64_t)front.size() / 3, ref, mu.data(), s.data(), M, ehvi.data(),
                               _data(partials)),
                    "gpe_ehvi3_values");
            }

            /// Addition (include/gpe_cei.h, model/gp/cei.hpp): the LOG of the constrained expected improvement of every candidate
            /// under outputs of this model: out0 is the objective (maximised), con_outs the constraints, constraint k met when its
            /// output is >= thr[k]; all share sigma (limbo's GP with dim_out > 1: a cboptimizer constraint model).  with_ei == false
            /// (no feasible incumbent yet): the log-probability of feasibility alone, f_best is not read.  The means are k^T alpha
            /// plus the mean functor; sigma^2 is the clamped variance of the LATENT function, or, observation == true, with the
            /// kernel's noise added (what query() reports).  partials (may be null): M x (2 + 2 C) column-major, d/d mu0, d/d s0,
            /// d/d mu_k, d/d s_k; terms (may be null): M x (1 + C), log EI and each log Phi(u_k).  The model is not changed.  On the
            /// model's home device; no samples (the prior), a host-resident model below the batch crossover and kernels without
            /// device code: query_batch() and the host sum of the same definition.
            void log_constrained_ei(const std::vector<Eigen::VectorXd>& candidates, int out0, const std::vector<int>& con_outs,
                const std::vector<double>& thr, double f_best, double xi, bool with_ei, bool observation, std::vector<double>& logcei,
                std::vector<double>* partials = nullptr, std::vector<double>* terms = nullptr) const
            {
                const int64_t M = candidates.size();
                const int C = (int)con_outs.size();
                std::vector<int> outs(1, out0);
                outs.insert(outs.end(), con_outs.begin(), con_outs.end());
                if (thr.size() != con_outs.size() || C > GPE_CEI_MAX_CONSTRAINTS || !_outputs_ok(outs)
                    || gpe_logcei_values(nullptr, with_ei, f_best, xi, C, thr.data(), nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr) != GPE_OK)
                    throw std::invalid_argument("limbo_amd: log_constrained_ei(): bad argument (include/gpe_cei.h)");
                _zeroed(M, logcei, partials, 2 * outs.size(), terms, outs.size());
                if (M == 0)
                    return;
                if (_joint_on_host(M)) { // the objective's belief is column 0, the constraints' the columns behind it
                    std::vector<double> mu, sd;
                    _beliefs_of(candidates, outs, observation, mu, sd);
                    limbo_amd::cei_host::values(with_ei, f_best, xi, C, thr.data(), mu.data(), sd.data(), mu.data() + M, sd.data() + M, M, logcei.data(),
                        _data(terms), _data(partials));
                    return;
                }
                const std::vector<double> Xc = _joint_points(candidates), add = _mean_add(candidates, outs);
                _eng.check(gpe_logcei_batch(_eng.get(), with_ei, out0, f_best, xi, C, con_outs.data(), thr.data(), Xc.data(), M, add.data(),
                               observation ? _kernel_function.noise() : 0.0, logcei.data(), _data(terms), _data(partials), nullptr, nullptr),
                    "gpe_logcei_batch");
            }
            /// gpe_logcei_values through this model's engine handle (has_engine()): beliefs the caller computed (mu_c, s_c: M x C
            /// column-major)
            void logcei_values(bool with_ei, double f_best, double xi, const std::vector<double>& thr, const std::vector<double>& mu0,
                const std::vector<double>& s0, const std::vector<double>& mu_c, const std::vector<double>& s_c, std::vector<double>& logcei,
                std::vector<double>* partials = nullptr, std::vector<double>* terms = nullptr) const
            {
                const int64_t M = mu0.size();
                _zeroed(M, logcei, partials, 2 * (1 + thr.size()), terms, 1 + thr.size());
                _eng.check(gpe_logcei_values(_eng.get(), with_ei, f_best, xi, (int)thr.size(), thr.data(), mu0.data(), s0.data(), mu_c.data(), s_c.data(),
                               M, logcei.data(), _data(terms), _data(partials)),
                    "gpe_logcei_values");
            }

            /// Addition (include/gpe_mes.h, model/gp/mes.hpp): the LOG of the max-value entropy search of every candidate under the
            /// outputs `outs` of this model (all share sigma), against K sampled maxima per output: ystar is K x outs.size()
            /// column-major (limbo_amd::max_value_samples, acqui/mes.hpp).  One output: MES; several: MESMO, the sum over them.  The
            /// means are k^T alpha plus the mean functor; sigma^2 is the clamped variance of the LATENT function, or, observation ==
            /// true, with the kernel's noise added (what query() reports).  partials (may be null): M x 2 J column-major, d/d mu_j
            /// then d/d s_j; terms (may be null): M x J, the log of each output's MES.  The model is not changed.  On the model's
            /// home device; no samples (the prior), a host-resident model below the batch crossover and kernels without device
            /// code: query_batch() and the host sum of the same definition.
            void max_value_entropy(const std::vector<Eigen::VectorXd>& candidates, const std::vector<int>& outs, const std::vector<double>& ystar,
                bool observation, std::vector<double>& logmes, std::vector<double>* terms = nullptr, std::vector<double>* partials = nullptr) const
            {
                const int64_t M = candidates.size();
                const int J = (int)outs.size();
                const int K = J > 0 ? (int)(ystar.size() / (size_t)J) : 0;
                if (J < 1 || (size_t)K * (size_t)J != ystar.size() || !_outputs_ok(outs)
                    || gpe_mes_values(nullptr, J, K, ystar.data(), nullptr, nullptr, 0, nullptr, nullptr, nullptr) != GPE_OK)
                    throw std::invalid_argument("limbo_amd: max_value_entropy(): bad argument (include/gpe_mes.h)");
                _zeroed(M, logmes, partials, 2 * (size_t)J, terms, (size_t)J);
                if (M == 0)
                    return;
                if (_joint_on_host(M)) {
                    std::vector<double> mu, sd;
                    _beliefs_of(candidates, outs, observation, mu, sd);
                    limbo_amd::mes_host::values(J, K, ystar.data(), mu.data(), sd.data(), M, logmes.data(), _data(terms), _data(partials));
                    return;
                }
                const std::vector<double> Xc = _joint_points(candidates), add = _mean_add(candidates, outs);
                _eng.check(gpe_mes_batch(_eng.get(), J, outs.data(), K, ystar.data(), Xc.data(), M, add.data(), observation ? _kernel_function.noise() : 0.0,
                               logmes.data(), _data(terms), _data(partials), nullptr, nullptr),
                    "gpe_mes_batch");
            }
            /// gpe_mes_values through this model's engine handle (has_engine()): beliefs the caller computed (mu, s: M x J column-major)
            void mes_values(int J, const std::vector<double>& ystar, const std::vector<double>& mu, const std::vector<double>& s,
                std::vector<double>& logmes, std::vector<double>* terms = nullptr, std::vector<double>* partials = nullptr) const
            {
                const int64_t M = J > 0 ? (int64_t)(mu.size() / (size_t)J) : 0;
                _zeroed(M, logmes, partials, 2 * (size_t)J, terms, (size_t)J);
                _eng.check(gpe_mes_values(_eng.get(), J, J > 0 ? (int)(ystar.size() / (size_t)J) : 0, ystar.data(), mu.data(), s.data(), M, logmes.data(),
                               _data(terms), _data(partials)),
                    "gpe_mes_values");
            }

            /// Addition: the largest number of points one sample() / sample_argmax() / query_joint() call takes (gpe_joint_max_points);
            /// no bound for a model that lives on the host
            int64_t joint_max_points() const
            {
                if (_samples.size() == 0 || _res.on_host() || limbo_amd::device_kernel<KernelFunction>::kind == limbo_amd::KIND_HOST_K)
                    return std::numeric_limits<int64_t>::max();
                int64_t m = 0;
                _eng.check(gpe_joint_max_points(_eng.get(), &m), "gpe_joint_max_points");
                return m;
            }

            /// Addition (include/gpe_nei.h, model/gp/nei.hpp): the LOG of the noisy expected improvement of every candidate under
            /// output `out` (maximised): EI averaged over S joint posterior draws of the function at the `baseline` points, every
            /// draw with its own incumbent and the belief at the candidate conditioned on it — no incumbent taken from noisy
            /// observations.  Z: baseline.size() x S standard normals, column-major, the caller's (standard_normals()); jitter is
            /// added to the baseline's covariance (no hidden default; 1e-6 is the usual choice).  The means are k^T alpha plus
            /// the mean functor.  fplus (S), cvar (M, no clamp) and cmean (S x M column-major) may be null.  Returns 0, or the
            /// 1-based first non-positive pivot of the baseline's covariance — lognei is then all zero: raise jitter.  The model is
            /// not changed.  On the model's home device; no samples (the prior), a host-resident model below the batch crossover
            /// and kernels without device code: the same formulas on the host (nei_host), the candidates in chunks.
            int log_noisy_ei(const std::vector<Eigen::VectorXd>& candidates, const std::vector<Eigen::VectorXd>& baseline, const std::vector<double>& Z,
                int out, double jitter, double xi, std::vector<double>& lognei, std::vector<double>* fplus = nullptr,
                std::vector<double>* cvar = nullptr, std::vector<double>* cmean = nullptr) const
            {
                const int64_t M = candidates.size(), B = baseline.size();
                const int S = B > 0 ? (int)(Z.size() / (size_t)B) : 0;
                bool ok = B >= 1 && B <= GPE_NEI_MAX_BASELINE && S >= 1 && S <= GPE_NEI_MAX_SAMPLES && (size_t)S * (size_t)B == Z.size() && out >= 0
                    && out < _dim_out && jitter >= 0.0 && std::isfinite(jitter) && std::isfinite(xi);
                for (size_t i = 0; ok && i < Z.size(); ++i)
                    ok = std::isfinite(Z[i]);
                if (!ok)
                    throw std::invalid_argument("limbo_amd: log_noisy_ei(): bad argument (include/gpe_nei.h)");
                lognei.assign((size_t)M, 0.0);
                if (fplus)
                    fplus->assign((size_t)S, 0.0);
                if (cvar)
                    cvar->assign((size_t)M, 0.0);
                if (cmean)
                    cmean->assign((size_t)S * (size_t)M, 0.0);
                if (M == 0)
                    return 0;
                if (_joint_on_host(B + M))
                    return _host_noisy_ei(candidates, baseline, Z, S, out, jitter, xi, lognei.data(), _data(fplus), _data(cvar), _data(cmean));
                const std::vector<double> Xb = _joint_points(baseline), Xc = _joint_points(candidates);
                const std::vector<double> mb = _mean_add(baseline, {out}), ma = _mean_add(candidates, {out});
                return _eng.check(gpe_lognei_batch(_eng.get(), out, Xb.data(), B, mb.data(), jitter, Z.data(), S, xi, Xc.data(), M, ma.data(),
                                      lognei.data(), _data(fplus), nullptr, nullptr, _data(cvar), _data(cmean), S),
                    "gpe_lognei_batch");
            }

            /// Addition (include/gpe_pathwise.h, model/gp/pathwise.hpp): n_draws posterior draws per output as FUNCTIONS — pathwise
            /// conditioning on n_features random Fourier features.  The set is evaluated anywhere, any number of times, with its
            /// exact gradient in the point; one multi-right-hand-side solve here, no solve per point later, no cap on the points.
            /// Omega0 (n_features x Dw, row-major), phase (n_features), W (n_features x n_draws x dim_out) and E (samples x n_draws x
            /// dim_out; empty: zeros) in the layouts of gpe_pathwise.h: a deterministic function of (model, Omega0, phase, W, E).
            /// On the model's home device; a host-resident model (and a model without samples: the prior's paths, Phi w + m): on
            /// the host from matrixL() and limbo_amd::query_grad::dk_dv; kernels without device code: std::logic_error.
            using PathSet = limbo_amd::pathwise::PathSet;
            PathSet sample_paths(int n_features, int n_draws, const std::vector<double>& Omega0, const std::vector<double>& phase,
                const std::vector<double>& W, const std::vector<double>& E) const
            {
                constexpr int kind = limbo_amd::device_kernel<KernelFunction>::kind;
                if (kind == limbo_amd::KIND_HOST_K)
                    throw std::logic_error("limbo_amd: sample_paths(): this kernel has no device code, hence no spectral law and no derivative in the query point");
                const int64_t n = _samples.size();
                const int D = _dim_in, P = _dim_out, R = n_features, S = n_draws;
                const Eigen::VectorXd hp = _kernel_function.h_params();
                const int nk = (int)hp.size() - (Params::kernel::optimize_noise() ? 1 : 0);
                const int Dw = limbo_amd::pathwise::freq_dim(kind, nk, D);
                if (R < 1 || S < 1 || (int64_t)Omega0.size() < (int64_t)R * Dw || (int64_t)phase.size() < R || (int64_t)W.size() < (int64_t)R * S * P
                    || (!E.empty() && (int64_t)E.size() < n * S * P))
                    throw std::runtime_error("limbo_amd: sample_paths(): Omega0, phase, W or E is smaller than features x draws x dim_out asks for");
                auto mean = [this](const Eigen::VectorXd& v) { return Eigen::VectorXd(_mean_function(v, *this)); };
                if (n == 0 || _res.on_host()) {
                    const std::vector<double> X = _pack(_samples, 0, (size_t)n);
                    limbo_amd::pathwise::HostPaths h;
                    h.make(kind, hp.data(), nk, D, P, X.data(), n, n ? matrixL().data() : nullptr, _obs_mean.data(), _kernel_function.noise(), R, S,
                        Omega0.data(), phase.data(), W.data(), E.empty() ? nullptr : E.data());
                    return PathSet(std::move(h), mean);
                }
                gpe_paths ps = nullptr;
                _eng.check(gpe_paths_create(_eng.get(), R, S, Omega0.data(), phase.data(), W.data(), E.empty() ? nullptr : E.data(), &ps), "gpe_paths_create");
                return PathSet(ps, D, P, S, mean);
            }
            /// ... with everything from the seed: limbo_amd::pathwise::spectral_draws(kind, n_features, Dw, seed), W from
            /// standard_normals(.., seed + 1) and E from standard_normals(.., seed + 2)
            PathSet sample_paths(int n_features, int n_draws, uint64_t seed) const
            {
                constexpr int kind = limbo_amd::device_kernel<KernelFunction>::kind;
                if (kind == limbo_amd::KIND_HOST_K)
                    throw std::logic_error("limbo_amd: sample_paths(): this kernel has no device code, hence no spectral law and no derivative in the query point");
                const int nk = (int)_kernel_function.h_params().size() - (Params::kernel::optimize_noise() ? 1 : 0);
                const limbo_amd::pathwise::Spectral sp = limbo_amd::pathwise::spectral_draws(kind, n_features, limbo_amd::pathwise::freq_dim(kind, nk, _dim_in), seed);
                const size_t cols = (size_t)std::max(n_draws, 0) * (size_t)_dim_out;
                return sample_paths(n_features, n_draws, sp.Omega0, sp.phase, standard_normals((size_t)std::max(n_features, 0) * cols, seed + 1),
                    standard_normals(_samples.size() * cols, seed + 2));
            }

            int dim_in() const
            {
                assert(_dim_in != -1);
                return _dim_in;
            }
            int dim_out() const
            {
                assert(_dim_out != -1);
                return _dim_out;
            }
            const KernelFunction& kernel_function() const { return _kernel_function; }
            KernelFunction& kernel_function() { return _kernel_function; }
            const MeanFunction& mean_function() const { return _mean_function; }
            MeanFunction& mean_function() { return _mean_function; }

            Eigen::VectorXd max_observation() const
            {
                if (_observations.cols() > 1)
                    std::cout << "WARNING max_observation with multi dimensional observations doesn't make sense" << std::endl;
                return tools::make_vector(_observations.maxCoeff());
            }
            Eigen::VectorXd mean_observation() const
            {
                assert(_dim_out > 0);
                return _samples.size() > 0 ? _mean_observation : Eigen::VectorXd::Zero(_dim_out);
            }
            const Eigen::MatrixXd& mean_vector() const { return _mean_vector; }
            const Eigen::MatrixXd& obs_mean() const { return _obs_mean; }
            int nb_samples() const { return _samples.size(); }

            /// gp.hpp:241-252
            void recompute(bool update_obs_mean = true, bool update_full_kernel = true)
            {
                assert(!_samples.empty());
                if (update_obs_mean)
                    this->_compute_obs_mean();
                if (update_full_kernel)
                    this->_compute_full_kernel(); // re-sends obs_mean, X stays resident
                else
                    this->_compute_alpha();
            }

            /// gp.hpp:254-264: K^-1 from L, cached until K changes
            void compute_inv_kernel()
            {
                _need_device();
                _status_or(_eng.check(gpe_compute_inv_kernel(_eng.get()), "gpe_compute_inv_kernel"));
                _Kinv_on_device();
            }

            /// gp.hpp:267-282
            double compute_log_lik()
            {
                if (_res.on_host()) { // gp.hpp:267-282, the P-quirk kept: log det and n log 2 pi are not multiplied by dim_out
                    const int64_t n = _samples.size();
                    long double logdet = 0.0L;
                    for (int64_t i = 0; i < n; ++i)
                        logdet += std::log(_matrixL.data()[i + i * n]);
                    logdet *= 2;
                    double a = 0.0;
                    for (int p = 0; p < _dim_out; ++p)
                        for (int64_t i = 0; i < n; ++i)
                            a += _obs_mean(i, p) * _alpha(i, p);
                    _log_lik = -0.5 * a - 0.5 * logdet - 0.5 * n * std::log(2 * M_PI);
                    return _log_lik;
                }
                double ll = 0.0;
                _eng.check(gpe_log_lik(_eng.get(), &ll), "gpe_log_lik");
                _log_lik = ll;
                return _log_lik;
            }

            /// gp.hpp:285-311
            Eigen::VectorXd compute_kernel_grad_log_lik()
            {
                _need_device();
                const int T = _kernel_function.h_params_size();
                Eigen::VectorXd grad = Eigen::VectorXd::Zero(T);
                if (limbo_amd::device_kernel<KernelFunction>::kind != limbo_amd::KIND_HOST_K) {
                    _push_kernel();
                    _eng.check(gpe_log_lik_grad(_eng.get(), grad.data(), T, Params::kernel::optimize_noise() ? 1 : 0), "gpe_log_lik_grad");
                    _Kinv_on_device(); // the device computed and cached K^-1 (gp.hpp:289-291)
                    return grad;
                }
                // kernels without device code: w = alpha alpha^T - K^-1 from the device, d k / d theta from the functor
                if (!_inv_kernel_updated)
                    compute_inv_kernel();
                const Eigen::MatrixXd& Ki = _host_Kinv();
                const Eigen::MatrixXd& al = alpha();
                const size_t n = _samples.size();
                for (size_t i = 0; i < n; ++i)
                    for (size_t j = 0; j <= i; ++j) {
                        double w = -Ki(i, j);
                        for (int p = 0; p < _dim_out; ++p)
                            w += al(i, p) * al(j, p);
                        Eigen::VectorXd g = _kernel_function.grad(_samples[i], _samples[j], i, j);
                        const double f = (i == j) ? 0.5 * w : w;
                        for (int t = 0; t < T; ++t)
                            grad(t) += f * g(t);
                    }
                return grad;
            }

            /// gp.hpp:314-330.  obs_mean(:, p)^T K^-1(:, n) is alpha(n, p) (gp.hpp:608-610), so the sum
            /// needs no N x N read-back: grad = sum_n sum_p alpha(n, p) * mean.grad(x_n).row(p).
            /// K^-1 is still produced on the device so that inv_kernel_computed() changes as in the reference.
            Eigen::VectorXd compute_mean_grad_log_lik()
            {
                if (!_inv_kernel_updated)
                    compute_inv_kernel();
                const Eigen::MatrixXd& al = alpha();
                const size_t n = _samples.size();
                const int T = _mean_function.h_params_size();
                Eigen::VectorXd grad = Eigen::VectorXd::Zero(T);
                for (size_t m = 0; m < n; ++m) {
                    Eigen::MatrixXd gm = _mean_function.grad(_samples[m], *this);
                    for (int p = 0; p < _dim_out; ++p)
                        for (int t = 0; t < T; ++t)
                            grad(t) += al(m, p) * gm(p, t);
                }
                return grad;
            }

            double get_log_lik() const { return _log_lik; }
            void set_log_lik(double log_lik) { _log_lik = log_lik; }

            /// gp.hpp:339-351 on the device (K^-1 diagonal and alpha never leave HBM)
            double compute_log_loo_cv()
            {
                _need_device();
                double v = 0.0;
                _eng.check(gpe_log_loo_cv(_eng.get(), &v), "gpe_log_loo_cv");
                _Kinv_on_device(); // gp.hpp:342-344
                _log_loo_cv = v;
                return _log_loo_cv;
            }

            /// gp.hpp:354-402.  The reference forms K^-1 dK_j, (K^-1 dK_j) alpha and (K^-1 dK_j) K^-1 for every
            /// hyper-parameter j; both terms of :389 are linear in dK_j, so the device builds ONE weight matrix
            /// W (one N^3 product, limbo_amd/csrc/grad.hip) and the gradient is sum_ab W_ab dK_j,ab.
            Eigen::VectorXd compute_kernel_grad_log_loo_cv()
            {
                _need_device();
                const int T = _kernel_function.h_params_size();
                Eigen::VectorXd grad = Eigen::VectorXd::Zero(T);
                if (limbo_amd::device_kernel<KernelFunction>::kind != limbo_amd::KIND_HOST_K) {
                    _push_kernel();
                    _eng.check(gpe_log_loo_cv_grad(_eng.get(), grad.data(), T, Params::kernel::optimize_noise() ? 1 : 0), "gpe_log_loo_cv_grad");
                    _Kinv_on_device();
                    return grad;
                }
                // kernels without device code: W from the device, d k / d theta from the functor
                const size_t n = _samples.size();
                Eigen::MatrixXd W(n, n);
                _eng.check(gpe_get_loo_weights(_eng.get(), W.data(), (int64_t)n), "gpe_get_loo_weights");
                _Kinv_on_device();
                for (size_t i = 0; i < n; ++i)
                    for (size_t j = 0; j <= i; ++j) {
                        Eigen::VectorXd g = _kernel_function.grad(_samples[i], _samples[j], i, j);
                        const double f = (i == j) ? W(i, j) : 2.0 * W(i, j);
                        for (int t = 0; t < T; ++t)
                            grad(t) += f * g(t);
                    }
                return grad;
            }
            double get_log_loo_cv() const { return _log_loo_cv; }
            void set_log_loo_cv(double v) { _log_loo_cv = v; }

            const Eigen::MatrixXd& matrixL() const
            {
                std::lock_guard<std::mutex> lk(_mirror_mu);
                if (_res.L_stale()) {
                    const int64_t n = _samples.size();
                    _matrixL.resize(n, n);
                    _eng.check(gpe_get_L(_eng.get(), _matrixL.data(), n), "gpe_get_L");
                    _res.L_fetched();
                }
                return _matrixL;
            }
            const Eigen::MatrixXd& alpha() const
            {
                std::lock_guard<std::mutex> lk(_mirror_mu);
                if (_res.alpha_stale()) {
                    _alpha.resize(_samples.size(), _dim_out);
                    _eng.check(gpe_get_alpha(_eng.get(), _alpha.data()), "gpe_get_alpha");
                    _res.alpha_fetched();
                }
                return _alpha;
            }
            const std::vector<Eigen::VectorXd>& samples() const { return _samples; }
            std::vector<Eigen::VectorXd> observations() const
            {
                std::vector<Eigen::VectorXd> obs;
                for (int i = 0; i < (int)_observations.rows(); ++i) {
                    Eigen::VectorXd o(_dim_out);
                    for (int p = 0; p < _dim_out; ++p)
                        o(p) = _observations(i, p);
                    obs.push_back(o);
                }
                return obs;
            }
            const Eigen::MatrixXd& observations_matrix() const { return _observations; }
            bool inv_kernel_computed() { return _inv_kernel_updated; }

            /// 0, or the 1-based index of the first non-positive Cholesky pivot of the last factorisation
            int last_status() const { return _status; }

            /// gp.hpp:439-460: any archive with save(vector / matrix / vector-of-vectors, name)
            template <typename A>
            void save(const std::string& directory) const
            {
                A archive(directory);
                save(archive);
            }
            template <typename A>
            void save(const A& archive) const
            {
                if (_kernel_function.h_params_size() > 0)
                    archive.save(_kernel_function.h_params(), "kernel_params");
                if (_mean_function.h_params_size() > 0)
                    archive.save(_mean_function.h_params(), "mean_params");
                archive.save(_samples, "samples");
                archive.save(_observations, "observations");
                archive.save(matrixL(), "matrixL");
                archive.save(alpha(), "alpha");
            }
            /// gp.hpp:462-511
            template <typename A>
            void load(const std::string& directory, bool recompute = true)
            {
                A archive(directory);
                load(archive, recompute);
            }
            template <typename A>
            void load(const A& archive, bool recompute = true)
            {
                _samples.clear();
                archive.load(_samples, "samples");
                archive.load(_observations, "observations");
                _adopt_dims((int)_samples[0].size(), (int)_observations.cols(), true);
                if (_kernel_function.h_params_size() > 0) {
                    Eigen::VectorXd h_params;
                    archive.load(h_params, "kernel_params");
                    assert(h_params.size() == (int)_kernel_function.h_params_size());
                    _kernel_function.set_h_params(h_params);
                }
                if (_mean_function.h_params_size() > 0) {
                    Eigen::VectorXd h_params;
                    archive.load(h_params, "mean_params");
                    assert(h_params.size() == (int)_mean_function.h_params_size());
                    _mean_function.set_h_params(h_params);
                }
                _update_mean_observation();
                _res.return_to_full_path();
                if (recompute)
                    this->recompute(true, true);
                else { // trust the stored factor: upload L and alpha (the block inverses are rebuilt on the device)
                    this->_compute_obs_mean();
                    archive.load(_matrixL, "matrixL");
                    archive.load(_alpha, "alpha");
                    if (_use_host((int64_t)_samples.size())) { // a small model stays where single-point calls are cheapest
                        _res.alpha_recomputed_on_host(); // (the stored alpha and factor are the host model)
                        _host_factor(true);
                        return;
                    }
                    _push_data();
                    _push_kernel();
                    _eng.check(gpe_set_L(_eng.get(), _matrixL.data(), _matrixL.rows()), "gpe_set_L");
                    _eng.check(gpe_set_alpha(_eng.get(), _alpha.data()), "gpe_set_alpha");
                    _factor_uploaded();
                }
            }

        protected:
            int _dim_in;
            int _dim_out;

            KernelFunction _kernel_function;
            MeanFunction _mean_function;

            std::vector<Eigen::VectorXd> _samples;
            Eigen::MatrixXd _observations;
            Eigen::MatrixXd _mean_vector;
            Eigen::MatrixXd _obs_mean;

            mutable Eigen::MatrixXd _alpha; // host mirror of the device's alpha
            Eigen::VectorXd _mean_observation;

            mutable Eigen::MatrixXd _kernel, _inv_kernel; // _kernel: host K (HOST_K kernels only); _inv_kernel: mirror

            mutable Eigen::MatrixXd _matrixL; // host mirror of the device's L

            double _log_lik, _log_loo_cv;
            bool _inv_kernel_updated;

            HyperParamsOptimizer _hp_optimize;

            // ---- device side -------------------------------------------------------------------
            mutable limbo_amd::Engine _eng;
            int _status = 0;
            mutable limbo_amd::Residency _res; // where the model lives, which mirrors are current (gp/residency.hpp); mutable: the mirrors
            mutable std::mutex _mirror_mu;     // and the shadow of a host model are filled from const calls
            mutable limbo_amd::QueryReplicas _replicas; // (gp/replicas.hpp) never copied with the GP

            bool _use_host(int64_t n) const { return _res.use_host(n, (int64_t)limbo_amd::min_n_for_gpu<Params>()); }
            /// everything without a host form: the model moves to the device and stays there
            void _need_device()
            {
                if (_res.leave_host_for_good() && !_samples.empty())
                    _compute_full_kernel();
            }

            // ---- the events that move _inv_kernel_updated (the reference's member) together with _res: one site each ----
            void _host_factor(bool built) // gp.hpp:570 / :602
            {
                built ? _res.factor_built_on_host() : _res.factor_updated_on_host();
                _inv_kernel_updated = false;
            }
            void _device_factor() // gp.hpp:570 / :602
            {
                _res.factor_changed_on_device();
                _inv_kernel_updated = false;
            }
            void _factor_uploaded()
            {
                _res.factor_uploaded();
                _inv_kernel_updated = false;
            }
            void _Kinv_on_device()
            {
                _res.Kinv_produced_on_device();
                _inv_kernel_updated = true;
            }
            void _emptied()
            {
                _res.emptied();
                _inv_kernel_updated = false;
            }

            void _swap(GP& o)
            {
                std::swap(_dim_in, o._dim_in);
                std::swap(_dim_out, o._dim_out);
                std::swap(_kernel_function, o._kernel_function);
                std::swap(_mean_function, o._mean_function);
                std::swap(_samples, o._samples);
                std::swap(_observations, o._observations);
                std::swap(_mean_vector, o._mean_vector);
                std::swap(_obs_mean, o._obs_mean);
                std::swap(_alpha, o._alpha);
                std::swap(_mean_observation, o._mean_observation);
                std::swap(_kernel, o._kernel);
                std::swap(_inv_kernel, o._inv_kernel);
                std::swap(_matrixL, o._matrixL);
                std::swap(_log_lik, o._log_lik);
                std::swap(_log_loo_cv, o._log_loo_cv);
                std::swap(_inv_kernel_updated, o._inv_kernel_updated);
                std::swap(_eng, o._eng);
                std::swap(_status, o._status);
                std::swap(_res, o._res); // (whole: a swap, unlike a copy, keeps "data on the device" and the shadow with their handle)
                _replicas.clear();       // (replicas belong to a handle; both handles changed hands)
                o._replicas.clear();
            }

            void _adopt_dims(int dim_in, int dim_out, bool always = false)
            {
                if (always || _dim_in != dim_in) {
                    _dim_in = dim_in;
                    _kernel_function = KernelFunction(_dim_in);
                }
                if (always || _dim_out != dim_out) {
                    _dim_out = dim_out;
                    _mean_function = MeanFunction(_dim_out);
                }
            }

            /// points [lo, hi) of pts as row-major doubles, the engine's layout
            std::vector<double> _pack(const std::vector<Eigen::VectorXd>& pts, size_t lo, size_t hi) const
            {
                std::vector<double> X((hi - lo) * (size_t)_dim_in);
                for (size_t i = lo; i < hi; ++i) {
                    assert((int)pts[i].size() == _dim_in);
                    std::copy(pts[i].data(), pts[i].data() + _dim_in, X.begin() + (i - lo) * (size_t)_dim_in);
                }
                return X;
            }

            void _status_or(int rc)
            {
                if (rc > 0)
                    _status = rc;
            }

            void _update_mean_observation()
            {
                _mean_observation = Eigen::VectorXd::Zero(_dim_out);
                const int n = _observations.rows();
                for (int p = 0; p < _dim_out; ++p) {
                    double s = 0.0;
                    for (int i = 0; i < n; ++i)
                        s += _observations(i, p);
                    _mean_observation(p) = n > 0 ? s / n : 0.0;
                }
            }

            /// gp.hpp:537-548 — host, by design
            void _compute_obs_mean()
            {
                assert(!_samples.empty());
                _mean_vector.resize(_samples.size(), _dim_out);
                _obs_mean.resize(_samples.size(), _dim_out);
                for (int i = 0; i < (int)_mean_vector.rows(); i++) {
                    assert((int)_samples[i].size() == _dim_in);
                    Eigen::VectorXd m = _mean_function(_samples[i], *this);
                    for (int p = 0; p < _dim_out; ++p) {
                        _mean_vector(i, p) = m(p);
                        _obs_mean(i, p) = _observations(i, p) - m(p);
                    }
                }
            }

            /// X and obs_mean to the device (const: a host model's shadow is filled from const calls; they do not raise data_pushed)
            void _send_data() const
            {
                const std::vector<double> X = _pack(_samples, 0, _samples.size());
                _eng.check(gpe_set_data(_eng.get(), X.data(), (int64_t)_samples.size(), _dim_in, _obs_mean.data(), _dim_out), "gpe_set_data");
            }
            void _push_data()
            {
                _send_data();
                _res.data_pushed();
            }

            /// kernel.hpp:116-123 on the device: log-space parameters (without the noise entry) + sigma_n^2
            void _send_kernel(const Eigen::VectorXd& hp, double noise) const
            {
                constexpr int kind = limbo_amd::device_kernel<KernelFunction>::kind;
                const bool functor_built = kind == limbo_amd::KIND_HOST_K; // (K and k* come from the host: no parameters to send)
                const int nk = functor_built ? 0 : (int)hp.size() - (Params::kernel::optimize_noise() ? 1 : 0);
                _eng.check(gpe_set_kernel(_eng.get(), kind, functor_built ? nullptr : hp.data(), nk, noise), "gpe_set_kernel");
            }
            void _push_kernel() { _send_kernel(_kernel_function.h_params(), _kernel_function.noise()); }

            /// gp.hpp:550-571: K -> L -> alpha, all on the device
            void _compute_full_kernel()
            {
                if (_use_host((int64_t)_samples.size())) {
                    _host_full_kernel();
                    return;
                }
                _res.moved_to_device();
                _stage_full_kernel();
                _commit_full_kernel(_eng.check(gpe_compute(_eng.get()), "gpe_compute"));
            }

            /// gp.hpp:550-571 on the host: K (lower, +noise+1e-8 on the diagonal through the functor's i == j) -> L -> alpha
            void _host_full_kernel()
            {
                const int64_t n = _samples.size();
                _matrixL.resize(n, n);
                double* L = _matrixL.data();
                for (int64_t j = 0; j < n; ++j)
                    for (int64_t i = j; i < n; ++i)
                        L[i + j * n] = _kernel_function(_samples[i], _samples[j], i, j);
                _status = limbo_amd::host_small::llt_lower(L, n, n);
                _host_alpha();
                _host_factor(true);
            }
            /// gp.hpp:605-611 on the host
            void _host_alpha()
            {
                const int64_t n = _samples.size();
                _alpha = _obs_mean;
                limbo_amd::host_small::solve_lower(_matrixL.data(), n, n, _alpha.data(), _dim_out, n);
                limbo_amd::host_small::solve_lower_t(_matrixL.data(), n, n, _alpha.data(), _dim_out, n);
                _res.alpha_recomputed_on_host();
            }
            /// gp.hpp:613-632 on the host: kta[p * ldk] = k*^T alpha_p, *var = k(v, v) - |L^-1 k*|^2 (before mean / clamp / noise)
            void _host_query(const Eigen::VectorXd& v, double* kta, int64_t ldk, double* var) const
            {
                const int64_t n = _samples.size();
                std::vector<double> k((size_t)n);
                for (int64_t i = 0; i < n; ++i)
                    k[(size_t)i] = _kernel_function(_samples[i], v);
                if (kta)
                    for (int p = 0; p < _dim_out; ++p) {
                        double s = 0.0;
                        const double* a = _alpha.data() + (int64_t)p * n;
                        for (int64_t i = 0; i < n; ++i)
                            s += k[(size_t)i] * a[i];
                        kta[(int64_t)p * ldk] = s;
                    }
                if (var) {
                    limbo_amd::host_small::solve_lower(_matrixL.data(), n, n, k.data(), 1, n);
                    double zz = 0.0;
                    for (int64_t i = 0; i < n; ++i)
                        zz += k[(size_t)i] * k[(size_t)i];
                    *var = _kernel_function(v, v) - zz;
                }
            }
            /// (host mode) the device copy behind large query_batch() calls: the same data and hyper-parameters factored on
            /// the device — equal to the host factor to rounding.  const: batched queries are const and may come from several
            /// threads (multi_gp.hpp:191-195); the refresh is serialised, the queries are by the handle's own lock.
            void _sync_device_shadow() const
            {
                std::lock_guard<std::mutex> lk(_mirror_mu);
                // the shadow is the HOST model on the device — its factor and alpha as they are (uploaded, not
                // re-factored) and the kernel's CURRENT hyper-parameters for k*.  After kernel_function().set_h_params()
                // without recompute() the reference answers queries with the old L / alpha and the new k* (gp.hpp:613-632);
                // so do the host loop and, now, this copy — whichever side of host_batch_crossover a batch falls on.
                const Eigen::VectorXd hp = _kernel_function.h_params();
                const double nz = _kernel_function.noise();
                std::vector<double> hpv(hp.data(), hp.data() + hp.size());
                if (_res.shadow_current(hpv, nz))
                    return;
                if (!_res.shadow_valid())
                    _send_data();
                _send_kernel(hp, nz);
                // (the factor goes up with every kernel change too: gpe_set_L also refreshes the Lambda^T x rows of SE-ARD with
                // Lambda columns, which depend on the hyper-parameters — n < min_n_for_gpu: a few hundred KB)
                _eng.check(gpe_set_L(_eng.get(), _matrixL.data(), _matrixL.rows()), "gpe_set_L");
                _eng.check(gpe_set_alpha(_eng.get(), _alpha.data()), "gpe_set_alpha");
                _res.shadow_refreshed(std::move(hpv), nz);
            }

        public:
            /// Addition: this model lives on the host (below Params::gpu::min_n_for_gpu samples, nothing device-only asked yet)
            bool host_resident() const { return _res.on_host() && _use_host((int64_t)_samples.size()); }

            /// Additions: the two halves of `_compute_full_kernel` around the device factorisation, so that a caller
            /// holding several independent GPs (model::MultiGP: one per output, multi_gp.hpp:124-126) can run all their
            /// factorisations as ONE batched launch sequence (`compute_full_kernels_batched` -> gpe_batch_compute).
            void _stage_full_kernel()
            {
                if (_res.on_host()) // (the batched callers: this object computes on the device from here on)
                    _res.leave_host_for_good();
                if (!_res.data_on_device())
                    _push_data();
                else
                    _eng.check(gpe_set_obs_mean(_eng.get(), _obs_mean.data()), "gpe_set_obs_mean");
                _push_kernel();
                if (limbo_amd::device_kernel<KernelFunction>::kind == limbo_amd::KIND_HOST_K) {
                    const size_t n = _samples.size();
                    _kernel.resize(n, n);
                    for (size_t i = 0; i < n; i++)
                        for (size_t j = 0; j <= i; ++j) {
                            _kernel(i, j) = _kernel_function(_samples[i], _samples[j], i, j);
                            _kernel(j, i) = _kernel(i, j);
                        }
                    _eng.check(gpe_set_K_host(_eng.get(), _kernel.data(), n), "gpe_set_K_host");
                }
            }
            void _commit_full_kernel(int status)
            {
                _status = status;
                _device_factor();
            }
            /// `_compute_full_kernel()` of every GP in `gps` (data already set: compute(samples, obs, false) or an earlier
            /// compute): GPs on the same device are stepped together by gpe_batch_compute (one launch sequence,
            /// gridDim.z = GP, when they agree in shape; the engine falls back to per-GP chains otherwise)
            static void compute_full_kernels_batched(const std::vector<GP*>& gps)
            {
                std::vector<int> devs;
                for (GP* g : gps) {
                    g->_stage_full_kernel();
                    if (std::find(devs.begin(), devs.end(), g->device()) == devs.end())
                        devs.push_back(g->device());
                }
                limbo::tools::par::loop(0, devs.size(), [&](size_t di) { // one host thread per device
                    std::vector<GP*> mine;
                    std::vector<gpe_handle> hs;
                    for (GP* g : gps)
                        if (g->device() == devs[di]) {
                            mine.push_back(g);
                            hs.push_back(g->_eng.get());
                        }
                    std::vector<int> st(hs.size(), 0);
                    const int rc = gpe_batch_compute(hs.data(), (int)hs.size(), st.data());
                    for (size_t i = 0; i < mine.size(); ++i)
                        mine[i]->_commit_full_kernel(mine[i]->_eng.check(st[i] < 0 ? st[i] : (rc < 0 ? rc : st[i]), "gpe_batch_compute"));
                });
            }

            /// Addition: one KernelLFOptimization evaluation (kernel_lf_opt.hpp:77-92: recompute(false), log-lik and, with
            /// want_grad, its gradient) of EVERY GP in `gps`, each with the hyper-parameters its kernel functor currently
            /// holds — the restarts of opt::ParallelRepeater or the outputs of multi_gp::ParallelLFOpt in lock-step.  GPs
            /// on the same device go through ONE gpe_batch_hp_objective (one launch sequence when they agree in shape).
            static void hp_objectives_batched(const std::vector<GP*>& gps, bool want_grad, std::vector<double>& liks,
                                              std::vector<Eigen::VectorXd>& grads)
            {
                const size_t G = gps.size();
                liks.assign(G, 0.0);
                grads.assign(G, Eigen::VectorXd());
                if (G == 0)
                    return;
                constexpr int kind = limbo_amd::device_kernel<KernelFunction>::kind;
                if (kind == limbo_amd::KIND_HOST_K) { // functor-built K: one by one (the factorisations still run on the device)
                    limbo::tools::par::loop(0, G, [&](size_t i) {
                        gps[i]->recompute(false);
                        liks[i] = gps[i]->compute_log_lik();
                        if (want_grad)
                            grads[i] = gps[i]->compute_kernel_grad_log_lik();
                    });
                    return;
                }
                const bool on = Params::kernel::optimize_noise();
                std::vector<int> devs;
                for (GP* g : gps) {
                    if (g->_res.on_host() || !g->_res.pinned()) { // lock-step restarts / outputs run on the device, the data re-sent
                        g->_res.leave_host_for_good();
                        g->_res.return_to_full_path();
                    }
                    if (!g->_res.data_on_device())
                        g->_push_data();
                    if (std::find(devs.begin(), devs.end(), g->device()) == devs.end())
                        devs.push_back(g->device());
                }
                limbo::tools::par::loop(0, devs.size(), [&](size_t di) { // one host thread per device
                    std::vector<size_t> mine;
                    std::vector<gpe_handle> hs;
                    for (size_t i = 0; i < G; ++i)
                        if (gps[i]->device() == devs[di]) {
                            mine.push_back(i);
                            hs.push_back(gps[i]->_eng.get());
                        }
                    const int T = gps[mine[0]]->_kernel_function.h_params_size();
                    const int nk = T - (on ? 1 : 0);
                    std::vector<double> th((size_t)nk * mine.size()), nz(mine.size()), lk(mine.size()), gr((size_t)T * mine.size());
                    for (size_t q = 0; q < mine.size(); ++q) {
                        const Eigen::VectorXd hp = gps[mine[q]]->_kernel_function.h_params();
                        for (int t = 0; t < nk; ++t)
                            th[q * nk + t] = hp(t);
                        nz[q] = gps[mine[q]]->_kernel_function.noise();
                    }
                    std::vector<int> st(mine.size(), 0);
                    const int rc = gpe_batch_hp_objective(hs.data(), (int)hs.size(), kind, th.data(), nk, nz.data(), on ? 1 : 0,
                                                          want_grad ? 1 : 0, lk.data(), want_grad ? gr.data() : nullptr, st.data());
                    for (size_t q = 0; q < mine.size(); ++q) {
                        GP* g = gps[mine[q]];
                        g->_commit_full_kernel(g->_eng.check(st[q] < 0 ? st[q] : (rc < 0 ? rc : st[q]), "gpe_batch_hp_objective"));
                        g->_log_lik = lk[q];
                        liks[mine[q]] = lk[q];
                        if (want_grad) {
                            g->_Kinv_on_device(); // the device computed and cached K^-1 (gp.hpp:289-291)
                            grads[mine[q]] = Eigen::VectorXd::Zero(T);
                            for (int t = 0; t < T; ++t)
                                grads[mine[q]](t) = gr[q * T + t];
                        }
                    }
                });
            }

        protected:

            /// One update of the factor after _samples changed from n0 rows (the factor _matrixL / the device still holds): on the
            /// host (host_step builds the new _matrixL; alpha follows) when the model lives there and stays there; through the full
            /// path, which decides where the model lives, when it crosses the threshold, its K is functor-built, its data is not
            /// on the device or it was empty; else on the device (device_step: the engine call, its status returned).
            template <typename HostStep, typename DeviceStep>
            void _update_factor(int64_t n0, HostStep host_step, DeviceStep device_step)
            {
                const int64_t n1 = _samples.size();
                if (_res.on_host() && _use_host(n1) && n0 >= 1 && (int64_t)_matrixL.rows() == n0) {
                    host_step();
                    _host_alpha();
                    _host_factor(false);
                    return;
                }
                if (_res.on_host() || _use_host(n1) || limbo_amd::device_kernel<KernelFunction>::kind == limbo_amd::KIND_HOST_K
                    || !_res.data_on_device() || n0 == 0) {
                    _res.return_to_full_path();
                    _compute_full_kernel();
                    return;
                }
                _push_kernel();
                _status_or(device_step());
                _device_factor();
            }

            /// gp.hpp:573-603 on the host for the rows n0 .. of _samples: L moves into the final-size matrix once, the rows follow
            /// one by one (host_small::append_row)
            void _host_append_rows(int64_t n0)
            {
                const int64_t n1 = _samples.size();
                Eigen::MatrixXd L2 = Eigen::MatrixXd::Zero(n1, n1);
                for (int64_t j = 0; j < n0; ++j) {
                    const double* src = _matrixL.data() + j * n0;
                    double* dst = L2.data() + j * n1;
                    for (int64_t i = j; i < n0; ++i)
                        dst[i] = src[i];
                }
                std::vector<double> kcol((size_t)n1), row((size_t)n1);
                int bad = 0;
                for (int64_t n = n0; n < n1; ++n) {
                    for (int64_t i = 0; i < n; ++i)
                        kcol[(size_t)i] = _kernel_function(_samples[i], _samples[n], i, n);
                    const double knn = _kernel_function(_samples[n], _samples[n], n, n);
                    const int b = limbo_amd::host_small::append_row(L2.data(), n, n1, kcol.data(), knn, row.data());
                    for (int64_t j = 0; j <= n; ++j)
                        L2.data()[n + j * n1] = row[(size_t)j];
                    if (b && !bad)
                        bad = b;
                }
                _matrixL = std::move(L2);
                if (bad)
                    _status = bad;
            }

            /// gp.hpp:573-603: one row appended to L (add_sample: the engine's single-row path)
            void _compute_incremental_kernel()
            {
                const int64_t n0 = (int64_t)_samples.size() - 1;
                _update_factor(n0, [&] { _host_append_rows(n0); }, [&] {
                    return _eng.check(gpe_add_sample(_eng.get(), _samples.back().data(), _dim_in, _obs_mean.data(), _dim_out), "gpe_add_sample");
                });
            }

            /// ... and the rows n0 .. of _samples at once (add_samples: the engine's blocked path, also for one row)
            void _compute_incremental_block(int64_t n0)
            {
                _update_factor(n0, [&] { _host_append_rows(n0); }, [&] {
                    const std::vector<double> X = _pack(_samples, (size_t)n0, _samples.size());
                    return _eng.check(gpe_add_samples(_eng.get(), X.data(), (int64_t)_samples.size() - n0, _dim_in, _obs_mean.data(), _dim_out), "gpe_add_samples");
                });
            }

            /// The factor after the rows R (ascending) left a model of n0 samples (remove_samples): on the host the same column
            /// sweep on _matrixL
            void _compute_removed(const std::vector<int64_t>& R, int64_t n0)
            {
                const int64_t n1 = _samples.size(), q = (int64_t)R.size();
                _update_factor(n0,
                    [&] {
                        Eigen::MatrixXd L2 = Eigen::MatrixXd::Zero(n1, n1);
                        limbo_amd::host_small::remove_rows(_matrixL.data(), n0, n0, R.data(), q, L2.data(), n1);
                        _matrixL = std::move(L2);
                    },
                    [&] {
                        _eng.check(gpe_remove_samples(_eng.get(), R.data(), q, _obs_mean.data(), _dim_out, GPE_REMOVE_AUTO), "gpe_remove_samples");
                        return 0; // (the update reports no pivot: last_status() keeps the factorisation's)
                    });
            }

            /// gp.hpp:605-611 with the existing factor
            void _compute_alpha()
            {
                if (_res.on_host()) {
                    _host_alpha();
                    return;
                }
                _eng.check(gpe_update_alpha(_eng.get(), _obs_mean.data()), "gpe_update_alpha");
                _res.alpha_changed_on_device();
            }

            const Eigen::MatrixXd& _host_Kinv() const
            {
                assert(!_res.on_host()); // (K^-1 only exists on the device: compute_inv_kernel() moved the model there)
                std::lock_guard<std::mutex> lk(_mirror_mu);
                if (_res.Kinv_stale()) {
                    const int64_t n = _samples.size();
                    _inv_kernel.resize(n, n);
                    _eng.check(gpe_get_Kinv(_eng.get(), _inv_kernel.data(), n), "gpe_get_Kinv");
                    _res.Kinv_fetched();
                }
                return _inv_kernel;
            }

            // kta[m + M p] = k*^T alpha_p ; var[m] = k(v,v) - |L^-1 k*|^2  (before mean / clamp / noise)
            void _query_many(const std::vector<Eigen::VectorXd>& pts, double* kta, double* var) const
            {
                const int64_t M = pts.size(), n = _samples.size();
                if (limbo_amd::device_kernel<KernelFunction>::kind != limbo_amd::KIND_HOST_K) {
                    const std::vector<double> Xq = _joint_points(pts);
                    // one GP's batch over ALL visible devices (gp/replicas.hpp); not when Params::gpu::device() pins the model
                    if (!_res.on_host() && limbo_amd::multi_device_query_min() > 0 && M >= (int64_t)limbo_amd::multi_device_query_min()
                        && limbo_amd::visible_devices() > 1 && limbo_amd::param_device<Params>::get() < 0)
                        _replicas.query(_eng, limbo_amd::visible_devices(), Xq.data(), M, _dim_in, _dim_out, kta, var);
                    else
                        _eng.check(gpe_query_batch(_eng.get(), Xq.data(), M, kta, var), "gpe_query_batch");
                    return;
                }
                if (_res.on_host())
                    _sync_device_shadow();
                // functor-built cross kernel (gp.hpp:626-632), solves on the device
                std::vector<double> Ks((size_t)(n * M)), zz((size_t)M);
                for (int64_t m = 0; m < M; ++m)
                    for (int64_t i = 0; i < n; ++i)
                        Ks[(size_t)(i + n * m)] = _kernel_function(_samples[i], pts[m]);
                _eng.check(gpe_query_batch_cross(_eng.get(), Ks.data(), M, kta, var ? zz.data() : nullptr), "gpe_query_batch_cross");
                if (var)
                    for (int64_t m = 0; m < M; ++m)
                        var[m] = _kernel_function(pts[m], pts[m]) - zz[(size_t)m];
            }
        public:
            /// Addition: give the per-device query replicas back (device memory: one copy of the model on every other device)
            void release_query_replicas() const { _replicas.clear(); }
            /// Addition (tests): how many devices the last large query_batch() was dealt over (1 + replicas alive)
            int query_devices() const { return _replicas.devices(); }
        protected:
            // ---- the joint posterior (query_joint, sample) ----
            bool _joint_on_host(int64_t M) const
            {
                if (_samples.size() == 0 || limbo_amd::device_kernel<KernelFunction>::kind == limbo_amd::KIND_HOST_K)
                    return true;
                return _res.on_host() && M * (int64_t)_samples.size() < (int64_t)limbo_amd::host_batch_crossover();
            }
            // row-major points for the engine (a host-resident model first refreshes its device copy)
            std::vector<double> _joint_points(const std::vector<Eigen::VectorXd>& pts) const
            {
                if (_res.on_host())
                    _sync_device_shadow();
                return _pack(pts, 0, pts.size());
            }
            // kta[m + M p], cov (M x M, column-major) on the host: the prior without samples, else from matrixL() and alpha()
            void _host_joint(const std::vector<Eigen::VectorXd>& pts, double* kta, double* cov, double jitter) const
            {
                const int64_t M = pts.size(), n = _samples.size();
                for (int64_t b = 0; b < M; ++b)
                    for (int64_t a = b; a < M; ++a) {
                        const double v = _kernel_function(pts[a], pts[b]) + (a == b ? jitter : 0.0);
                        cov[a + M * b] = v;
                        cov[b + M * a] = v;
                    }
                if (n == 0) {
                    if (kta)
                        std::fill(kta, kta + M * _dim_out, 0.0);
                    return;
                }
                const Eigen::MatrixXd& L = matrixL();
                const Eigen::MatrixXd& al = alpha();
                std::vector<double> Ks((size_t)(n * M));
                for (int64_t m = 0; m < M; ++m)
                    for (int64_t i = 0; i < n; ++i)
                        Ks[(size_t)(i + n * m)] = _kernel_function(_samples[i], pts[m]);
                if (kta)
                    for (int p = 0; p < _dim_out; ++p)
                        for (int64_t m = 0; m < M; ++m) {
                            double s = 0.0;
                            for (int64_t i = 0; i < n; ++i)
                                s += Ks[(size_t)(i + n * m)] * al.data()[i + n * p];
                            kta[m + M * p] = s;
                        }
                limbo_amd::host_small::solve_lower(L.data(), n, n, Ks.data(), M, n);
                for (int64_t b = 0; b < M; ++b)
                    for (int64_t a = b; a < M; ++a) {
                        double s = 0.0;
                        for (int64_t i = 0; i < n; ++i)
                            s += Ks[(size_t)(i + n * a)] * Ks[(size_t)(i + n * b)];
                        cov[a + M * b] -= s;
                        if (a != b)
                            cov[b + M * a] = cov[a + M * b];
                    }
            }
            // ---- the marginal beliefs of a batch under some outputs (expected_hypervolume_improvement, log_constrained_ei,
            // max_value_entropy) ----
            static double* _data(std::vector<double>* v) { return v ? v->data() : nullptr; }
            // are the outputs in range and distinct?
            bool _outputs_ok(const std::vector<int>& outs) const
            {
                for (size_t j = 0; j < outs.size(); ++j) {
                    if (outs[j] < 0 || outs[j] >= _dim_out)
                        return false;
                    for (size_t i = 0; i < j; ++i)
                        if (outs[i] == outs[j])
                            return false;
                }
                return true;
            }
            // size and zero what a call returns: one value per point, n_partials / n_terms columns where asked for
            static void _zeroed(int64_t M, std::vector<double>& values, std::vector<double>* partials, size_t n_partials, std::vector<double>* terms,
                size_t n_terms)
            {
                values.assign((size_t)M, 0.0);
                if (partials)
                    partials->assign(n_partials * (size_t)M, 0.0);
                if (terms)
                    terms->assign(n_terms * (size_t)M, 0.0);
            }
            // the host branch: query_batch(), then the means of outputs outs[j] and the standard deviation they share (the latent
            // function's, or the observation's), both M x J column-major
            void _beliefs_of(const std::vector<Eigen::VectorXd>& pts, const std::vector<int>& outs, bool observation, std::vector<double>& mu,
                std::vector<double>& sd) const
            {
                const size_t M = pts.size(), J = outs.size();
                const double noise = _kernel_function.noise();
                Eigen::MatrixXd m;
                Eigen::VectorXd s2;
                query_batch(pts, m, s2);
                mu.resize(M * J);
                sd.resize(M * J);
                for (size_t i = 0; i < M; ++i)
                    for (size_t j = 0; j < J; ++j) {
                        mu[i + M * j] = m(i, outs[j]);
                        sd[i + M * j] = std::sqrt(observation ? s2(i) : std::max(s2(i) - noise, 0.0));
                    }
            }
            // the device branch: the mean functor's outputs outs[j] at every point, M x J column-major
            std::vector<double> _mean_add(const std::vector<Eigen::VectorXd>& pts, const std::vector<int>& outs) const
            {
                const size_t M = pts.size();
                std::vector<double> add(M * outs.size());
                for (size_t m = 0; m < M; ++m) {
                    const Eigen::VectorXd mv = _mean_function(pts[m], *this);
                    for (size_t j = 0; j < outs.size(); ++j)
                        add[M * j + m] = mv(outs[j]);
                }
                return add;
            }
            // log_noisy_ei on the host: the baseline's covariance (B x B) and factor once, then the candidates in chunks of 512 — their
            // variances and the B x chunk cross-covariance alone, never the joint covariance of all B + M points.  No samples: the prior.
            int _host_noisy_ei(const std::vector<Eigen::VectorXd>& cand, const std::vector<Eigen::VectorXd>& base, const std::vector<double>& Z, int S,
                int out, double jitter, double xi, double* lognei, double* fplus, double* cvar, double* cmean) const
            {
                const int64_t M = cand.size(), B = base.size(), n = _samples.size();
                const double* al = n > 0 ? alpha().data() : nullptr;
                const double* L = n > 0 ? matrixL().data() : nullptr;
                // zs = L^-1 k(X, pts) (n x m) in place, mu[m] = k^T alpha_out + the mean functor, var (may be null) = k(v, v) - |z|^2
                auto solve = [&](const std::vector<Eigen::VectorXd>& pts, int64_t p0, int64_t m, std::vector<double>& zs, double* mu, double* var) {
                    zs.assign((size_t)(n * m), 0.0);
                    for (int64_t q = 0; q < m; ++q) {
                        const Eigen::VectorXd& v = pts[(size_t)(p0 + q)];
                        double s = 0.0;
                        for (int64_t i = 0; i < n; ++i) {
                            zs[(size_t)(i + n * q)] = _kernel_function(_samples[i], v);
                            s += zs[(size_t)(i + n * q)] * al[i + n * out];
                        }
                        mu[q] = s + _mean_function(v, *this)(out);
                    }
                    if (n > 0)
                        limbo_amd::host_small::solve_lower(L, n, n, zs.data(), m, n);
                    for (int64_t q = 0; q < m && var; ++q) {
                        double zz = 0.0;
                        for (int64_t i = 0; i < n; ++i)
                            zz += zs[(size_t)(i + n * q)] * zs[(size_t)(i + n * q)];
                        var[q] = _kernel_function(pts[(size_t)(p0 + q)], pts[(size_t)(p0 + q)]) - zz;
                    }
                };
                std::vector<double> zb, zc, mu_b((size_t)B), Sig((size_t)(B * B));
                solve(base, 0, B, zb, mu_b.data(), nullptr);
                for (int64_t b = 0; b < B; ++b)
                    for (int64_t a = b; a < B; ++a) {
                        double s = 0.0;
                        for (int64_t i = 0; i < n; ++i)
                            s += zb[(size_t)(i + n * a)] * zb[(size_t)(i + n * b)];
                        Sig[(size_t)(a + B * b)] = Sig[(size_t)(b + B * a)] = _kernel_function(base[(size_t)a], base[(size_t)b]) - s;
                    }
                limbo_amd::nei_host::Baseline bl;
                if (const int rc = limbo_amd::nei_host::prepare(Sig.data(), mu_b.data(), B, jitter, Z.data(), S, bl))
                    return rc;
                if (fplus)
                    std::copy(bl.fplus.begin(), bl.fplus.end(), fplus);
                const int64_t chunk = 512;
                std::vector<double> C((size_t)(B * std::min(chunk, M))), mu((size_t)std::min(chunk, M)), var((size_t)std::min(chunk, M));
                for (int64_t m0 = 0; m0 < M; m0 += chunk) {
                    const int64_t m = std::min(chunk, M - m0);
                    solve(cand, m0, m, zc, mu.data(), var.data());
                    for (int64_t q = 0; q < m; ++q)
                        for (int64_t b = 0; b < B; ++b) {
                            double s = 0.0;
                            for (int64_t i = 0; i < n; ++i)
                                s += zb[(size_t)(i + n * b)] * zc[(size_t)(i + n * q)];
                            C[(size_t)(b + B * q)] = _kernel_function(base[(size_t)b], cand[(size_t)(m0 + q)]) - s;
                        }
                    limbo_amd::nei_host::condition(bl, Z.data(), xi, C.data(), var.data(), mu.data(), m, lognei + m0, cvar ? cvar + m0 : nullptr,
                        cmean ? cmean + (int64_t)S * m0 : nullptr);
                }
                return 0;
            }
            // gpe_query_batch_grad's four outputs on the host, from matrixL() and alpha() and the kernel's derivative by (kind, log-theta)
            void _host_query_grad(const std::vector<Eigen::VectorXd>& pts, double* kta, double* var, double* dkta, double* dvar) const
            {
                const int64_t M = pts.size(), n = _samples.size();
                const int D = _dim_in, P = _dim_out;
                constexpr int kind = limbo_amd::device_kernel<KernelFunction>::kind;
                const Eigen::VectorXd hp = _kernel_function.h_params();
                const int nk = (int)hp.size() - (Params::kernel::optimize_noise() ? 1 : 0);
                const Eigen::MatrixXd& L = matrixL();
                const Eigen::MatrixXd& al = alpha();
                std::vector<double> k((size_t)n), w((size_t)n), dk((size_t)D);
                for (int64_t m = 0; m < M; ++m) {
                    assert((int)pts[m].size() == D);
                    for (int64_t i = 0; i < n; ++i)
                        k[(size_t)i] = _kernel_function(_samples[i], pts[m]);
                    for (int p = 0; p < P; ++p) {
                        double s = 0.0;
                        for (int64_t i = 0; i < n; ++i)
                            s += k[(size_t)i] * al.data()[i + n * p];
                        kta[m + M * p] = s;
                    }
                    w = k;
                    limbo_amd::host_small::solve_lower(L.data(), n, n, w.data(), 1, n);
                    double zz = 0.0;
                    for (int64_t i = 0; i < n; ++i)
                        zz += w[(size_t)i] * w[(size_t)i];
                    var[m] = _kernel_function(pts[m], pts[m]) - zz;
                    limbo_amd::host_small::solve_lower_t(L.data(), n, n, w.data(), 1, n); // w = K^-1 k
                    for (int q = 0; q < D * (P + 1); ++q)
                        (q < D * P ? dkta[m + M * q] : dvar[m + M * (q - D * P)]) = 0.0;
                    for (int64_t i = 0; i < n; ++i) {
                        limbo_amd::query_grad::dk_dv(kind, hp.data(), nk, D, pts[m].data(), _samples[i].data(), dk.data());
                        for (int d = 0; d < D; ++d) {
                            for (int p = 0; p < P; ++p)
                                dkta[m + M * (d + (int64_t)D * p)] += al.data()[i + n * p] * dk[(size_t)d];
                            dvar[m + M * d] -= 2.0 * w[(size_t)i] * dk[(size_t)d];
                        }
                    }
                }
            }
            // F (M x S x P, may be null), argmax / fmax (S x P, may be null)
            void _draws(const std::vector<Eigen::VectorXd>& pts, const std::vector<double>& Z, int S, double jitter, double* F, int64_t* argmax,
                double* fmax) const
            {
                const int64_t M = pts.size();
                const int P = _dim_out;
                if ((int64_t)Z.size() < M * S * P)
                    throw std::runtime_error("limbo_amd: sample(): Z must hold points x draws x dim_out standard normals");
                if (M == 0 || S <= 0)
                    return;
                std::vector<double> mq((size_t)(M * P));
                for (int64_t m = 0; m < M; ++m) {
                    Eigen::VectorXd mv = _mean_function(pts[m], *this);
                    for (int p = 0; p < P; ++p)
                        mq[(size_t)(m + M * p)] = mv(p);
                }
                int rc = 0;
                if (!_joint_on_host(M)) {
                    const std::vector<double> Xq = _joint_points(pts);
                    rc = _eng.check(gpe_joint_draws(_eng.get(), Xq.data(), M, jitter, mq.data(), Z.data(), S, F, argmax, fmax), "gpe_joint_draws");
                }
                else {
                    std::vector<double> kta((size_t)(M * P)), C((size_t)(M * M)), f((size_t)M);
                    _host_joint(pts, kta.data(), C.data(), jitter);
                    rc = limbo_amd::host_small::llt_lower(C.data(), M, M);
                    for (int q = 0; q < S * P && rc == 0; ++q) {
                        const int p = q / S;
                        const double* z = Z.data() + (int64_t)q * M;
                        for (int64_t m = 0; m < M; ++m) {
                            double s = 0.0;
                            for (int64_t j = 0; j <= m; ++j)
                                s += C[(size_t)(m + M * j)] * z[j];
                            f[(size_t)m] = mq[(size_t)(m + M * p)] + (kta[(size_t)(m + M * p)] + s);
                        }
                        if (F)
                            std::copy(f.begin(), f.end(), F + (int64_t)q * M);
                        int64_t best = 0;
                        for (int64_t m = 1; m < M; ++m)
                            if (f[(size_t)m] > f[(size_t)best])
                                best = m;
                        if (argmax)
                            argmax[q] = best;
                        if (fmax)
                            fmax[q] = f[(size_t)best];
                    }
                }
                if (rc > 0)
                    throw std::runtime_error("limbo_amd: sample(): cov + jitter I is not positive definite (pivot " + std::to_string(rc) + "): raise jitter");
            }
            void _query_one(const Eigen::VectorXd& v, Eigen::VectorXd* kta, double* var) const
            {
                if (_res.on_host()) {
                    if (kta)
                        kta->resize(_dim_out);
                    _host_query(v, kta ? kta->data() : nullptr, 1, var);
                    return;
                }
                std::vector<Eigen::VectorXd> one(1, v);
                std::vector<double> k((size_t)_dim_out);
                double vv = 0.0;
                _query_many(one, kta ? k.data() : nullptr, var ? &vv : nullptr);
                if (kta) {
                    kta->resize(_dim_out);
                    for (int p = 0; p < _dim_out; ++p)
                        (*kta)(p) = k[(size_t)p];
                }
                if (var)
                    *var = vv;
            }
            /// gp.hpp:613-616
            Eigen::VectorXd _finish_mu(const Eigen::VectorXd& v, const Eigen::VectorXd& kta) const
            {
                Eigen::VectorXd m = _mean_function(v, *this);
                for (int p = 0; p < _dim_out; ++p)
                    m(p) += kta(p);
                return m;
            }
            /// gp.hpp:621-623
            static double _finish_sigma(double res) { return (res <= std::numeric_limits<double>::epsilon()) ? 0 : res; }
        };

        template <typename Params>
        using GPBasic = GP<Params, kernel::MaternFiveHalves<Params>, mean::Data<Params>, gp::NoLFOpt<Params>>;

        template <typename Params>
        using GPOpt = GP<Params, kernel::SquaredExpARD<Params>, mean::Data<Params>, gp::KernelLFOpt<Params>>;
    } // namespace model
} // namespace limbo

#endif
