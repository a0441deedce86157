// limbo/acqui/thompson.hpp — Thompson sampling over a candidate set: batch proposals from ONE model state.
// Not in the reference (its acquisition functors score one point from the marginals, src/limbo/acqui/ucb.hpp:77-95); built
// on the joint posterior of model::GP (query_joint / sample, include/gpe_joint.h): q independent function draws over the
// candidates, each proposes its own maximiser.  A `boptimizer`-shaped loop evaluates the q proposals, brings them back with
// ONE model::GP::add_samples() (include/gpe_append.h: a blocked update, one alpha solve) — or add_sample() for each — and
// asks again.
// thompson_paths_batch: the same proposals from draws that are FUNCTIONS (model::GP::sample_paths, include/gpe_pathwise.h): each of
// the q paths is maximised over [0, 1]^D by a candidate cloud followed by a lock-step gradient search on the path itself — no
// candidate set to keep resident, no M x M covariance, and the maximum is found, not only its basin.
// Deterministic batches from the same model state (GP-BUCB, the kriging believer): acqui/batch_select.hpp.
#ifndef LIMBO_AMD_ACQUI_THOMPSON_HPP
#define LIMBO_AMD_ACQUI_THOMPSON_HPP
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <random>
#include <stdexcept>
#include <type_traits>
#include <vector>

#include <Eigen/Core>

#include <limbo/opt/batch_grad_search.hpp>

namespace limbo_amd {
    /// the default aggregator of limbo's optimisers (bayes_opt/bo_base.hpp: FirstElem): the first output
    struct FirstElem {
        typedef double result_type;
        double operator()(const Eigen::VectorXd& x) const { return x(0); }
    };

    /// The indices (into `candidates`) that maximise q independent posterior draws of afun(f(.)); the lowest index on exact
    /// ties.  Draw s uses the standard normals Model::standard_normals(M q dim_out, seed) in sample()'s layout, so the result
    /// equals the arg-max over model.sample(candidates, q, seed, jitter).  With one output and the FirstElem aggregator the
    /// arg-max runs on the device and the draws never leave it; otherwise they are aggregated on the host.
    /// jitter: as for sample() — the kernel's noise, or a small value (1e-8 .. 1e-6) for draws of f.
    template <typename Model, typename AggregatorFunction = FirstElem>
    std::vector<int64_t> thompson_batch(const Model& model, const std::vector<Eigen::VectorXd>& candidates, int q,
        const AggregatorFunction& afun = AggregatorFunction(), uint64_t seed = 0, double jitter = 1e-6)
    {
        const int64_t M = candidates.size();
        const int P = model.dim_out();
        std::vector<int64_t> out;
        if (M == 0 || q <= 0)
            return out;
        const std::vector<double> Z = Model::standard_normals((size_t)M * (size_t)q * (size_t)P, seed);
        if (P == 1 && std::is_same<AggregatorFunction, FirstElem>::value) {
            std::vector<double> fmax;
            model.sample_argmax(candidates, Z, q, jitter, out, fmax);
            return out;
        }
        const std::vector<Eigen::MatrixXd> F = model.sample(candidates, Z, q, jitter);
        for (int s = 0; s < q; ++s) {
            int64_t best = 0;
            double vbest = 0.0;
            for (int64_t m = 0; m < M; ++m) {
                Eigen::VectorXd row(P);
                for (int p = 0; p < P; ++p)
                    row(p) = F[(size_t)s](m, p);
                const double v = afun(row);
                if (m == 0 || v > vbest) {
                    vbest = v;
                    best = m;
                }
            }
            out.push_back(best);
        }
        return out;
    }

    /// q proposals in [0, 1]^D from ONE model state: q pathwise posterior draws (model.sample_paths(n_features, q, seed); one
    /// output, the FirstElem aggregator), each maximised on its own:
    ///   1. Params::opt_batchgradsearch::points() uniform candidates (std::mt19937_64(seed + 3)), ONE evaluation of all paths;
    ///   2. the best Params::opt_batchgradsearch::starts() candidates of every path advance through opt::rprop_lockstep
    ///      (Params::opt_rprop): each iteration is ONE eval_grad of all q x starts points.  eval_grad evaluates every path at every
    ///      point and each point keeps its own path's column — q times the work needed, on q x starts points only (a per-point path
    ///      index is not part of the interface);
    ///   3. per path the best point seen by any of its starts.  rprop_lockstep returns the best point SEEN, the start included, and a
    ///      point's value does not depend on the batch it is asked in, so proposal s is never worse on path s than that path's best
    ///      candidate.
    template <typename Params, typename Model>
    std::vector<Eigen::VectorXd> thompson_paths_batch(const Model& model, int q, uint64_t seed = 0, int n_features = 1024)
    {
        std::vector<Eigen::VectorXd> out;
        if (q <= 0)
            return out;
        if (model.dim_out() != 1)
            throw std::logic_error("limbo_amd: thompson_paths_batch(): one output (the FirstElem aggregator) only");
        const int D = model.dim_in();
        const int n = std::max(1, Params::opt_batchgradsearch::points());
        const size_t starts = (size_t)std::min(n, std::max(1, Params::opt_batchgradsearch::starts()));
        const auto paths = model.sample_paths(n_features, q, seed);
        std::mt19937_64 g(seed + 3);
        std::uniform_real_distribution<double> u01(0.0, 1.0);
        std::vector<Eigen::VectorXd> pts((size_t)n, Eigen::VectorXd(D));
        for (auto& p : pts)
            for (int d = 0; d < D; ++d)
                p(d) = u01(g);
        const std::vector<Eigen::MatrixXd> F = paths.eval(pts);
        std::vector<Eigen::VectorXd> inits;
        for (int s = 0; s < q; ++s) {
            std::vector<size_t> order((size_t)n);
            std::iota(order.begin(), order.end(), (size_t)0);
            const Eigen::MatrixXd& f = F[(size_t)s];
            std::partial_sort(order.begin(), order.begin() + starts, order.end(),
                [&](size_t a, size_t b) { return f(a, 0) > f(b, 0) || (f(a, 0) == f(b, 0) && a < b); });
            for (size_t j = 0; j < starts; ++j)
                inits.push_back(pts[order[j]]);
        }
        auto fb = [&](const std::vector<Eigen::VectorXd>& xs, bool) {
            std::vector<Eigen::MatrixXd> f, df;
            paths.eval_grad(xs, f, df);
            std::vector<limbo::opt::eval_t> v;
            for (size_t m = 0; m < xs.size(); ++m) {
                const size_t s = m / starts;
                Eigen::VectorXd gr(D);
                for (int d = 0; d < D; ++d)
                    gr(d) = df[s](m, d);
                v.push_back(limbo::opt::eval_t{f[s](m, 0), limbo::opt::eval_t::second_type(gr)});
            }
            return v;
        };
        const auto res = limbo::opt::rprop_lockstep<Params>(fb, inits, true);
        for (int s = 0; s < q; ++s) {
            size_t best = (size_t)s * starts;
            for (size_t j = 1; j < starts; ++j)
                if (res[(size_t)s * starts + j].second > res[best].second)
                    best = (size_t)s * starts + j;
            out.push_back(res[best].first);
        }
        return out;
    }
} // namespace limbo_amd
#endif
