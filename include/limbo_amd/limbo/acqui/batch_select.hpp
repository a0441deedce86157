// limbo/acqui/batch_select.hpp — deterministic batch proposals from ONE model state by greedy selection with hallucinated
// observations (model::GP::select_batch, include/gpe_batch_select.h).
// Not in the reference (its acquisition functors score one point from the marginals, src/limbo/acqui/ucb.hpp:77-95,
// src/limbo/acqui/ei.hpp:77-120).  Round by round: the candidate with the largest acquisition value is taken, the posterior
// VARIANCE of every candidate is conditioned on a noisy observation there — the mean cannot move, nothing has been observed —
// and the acquisition is scored again.  bucb_batch: acqui::UCB's value (GP-BUCB); believer_ei_batch: acqui::EI's (the kriging
// believer: the believed observation is the posterior mean, which leaves the mean where it is).  A `boptimizer`-shaped loop
// evaluates the q proposals, brings them back with ONE model::GP::add_samples() and asks again.  acqui/thompson.hpp proposes at
// random from the same model state.
// The first pick is the arg-max of acqui::UCB::batch / acqui::EI::batch over the candidates; the kernel's noise is both what the
// score adds to the variance (as query() does) and the noise of the hallucinated observations.
#ifndef LIMBO_AMD_ACQUI_BATCH_SELECT_HPP
#define LIMBO_AMD_ACQUI_BATCH_SELECT_HPP
#include <algorithm>
#include <cstdint>
#include <limits>
#include <type_traits>
#include <vector>

#include <Eigen/Core>

#include <limbo/acqui/ei.hpp>
#include <limbo/acqui/thompson.hpp>
#include <limbo/acqui/ucb.hpp>
#include <limbo/mean/constant.hpp>
#include <limbo/mean/data.hpp>
#include <limbo/mean/null_function.hpp>

#include "../../../gpe_batch_select.h"

namespace limbo_amd {
    /// mean functors whose value does not depend on the point: they shift every candidate's mean alike
    template <typename Mean>
    struct mean_is_constant : std::false_type {
    };
    template <typename P>
    struct mean_is_constant<limbo::mean::NullFunction<P>> : std::true_type {
    };
    template <typename P>
    struct mean_is_constant<limbo::mean::Constant<P>> : std::true_type {
    };
    template <typename P>
    struct mean_is_constant<limbo::mean::Data<P>> : std::true_type {
    };

    namespace batch_select_detail {
        // One output, the FirstElem aggregator and a constant mean: mu = k^T alpha + const, formed by select_batch itself (no
        // second pass over the candidates): `shift` is the constant, mu stays empty.  Otherwise mu[m] = afun(mu(v_m)) from one
        // query_batch, complete.
        template <typename Model, typename AggregatorFunction>
        bool means(const Model& model, const std::vector<Eigen::VectorXd>& candidates, const AggregatorFunction& afun, std::vector<double>& mu,
            double& shift)
        {
            using Mean = typename std::decay<decltype(model.mean_function())>::type;
            shift = 0.0;
            mu.clear();
            if (model.dim_out() == 1 && std::is_same<AggregatorFunction, FirstElem>::value && mean_is_constant<Mean>::value) {
                shift = model.mean_function()(candidates[0], model)(0);
                return true;
            }
            Eigen::MatrixXd m;
            Eigen::VectorXd s2;
            model.query_batch(candidates, m, s2);
            mu.resize(candidates.size());
            for (size_t i = 0; i < candidates.size(); ++i) {
                Eigen::VectorXd row(m.cols());
                for (int p = 0; p < (int)m.cols(); ++p)
                    row(p) = m(i, p);
                mu[i] = afun(row);
            }
            return false;
        }
    } // namespace batch_select_detail

    /// q indices into `candidates` by GP-BUCB: round t takes the arg-max of afun(mu) + Params::acqui_ucb::alpha() sqrt(sigma_t^2 +
    /// noise), sigma_t^2 conditioned on the t picks before it (the lowest index on exact ties).  distinct: no candidate twice.
    /// Fewer than q indices come back when a round's pivot is not positive (a candidate picked again without noise).
    template <typename Params, typename Model, typename AggregatorFunction = FirstElem>
    std::vector<int64_t> bucb_batch(const Model& model, const std::vector<Eigen::VectorXd>& candidates, int q,
        const AggregatorFunction& afun = AggregatorFunction(), bool distinct = true)
    {
        std::vector<int64_t> idx;
        std::vector<double> score, mu;
        if (candidates.empty() || q <= 0)
            return idx;
        double shift = 0.0; // (a constant shift of every mean does not move UCB's arg-max)
        batch_select_detail::means(model, candidates, afun, mu, shift);
        const double noise = model.kernel_function().noise();
        const int rc = model.select_batch(candidates, q, GPE_SELECT_UCB, Params::acqui_ucb::alpha(), mu, noise, noise, distinct, idx, score);
        if (rc > 0)
            idx.resize((size_t)(rc - 1)); // (round rc - 1 was picked but could not be conditioned on: it is a replicate of an earlier one)
        return idx;
    }

    /// q indices into `candidates` by the kriging believer on expected improvement: round t takes the arg-max of acqui::EI's value
    /// with f+ = the best predicted mean over the samples (one query_batch, as acqui::EI) and Params::acqui_ei::jitter().  Without
    /// samples EI is 0 everywhere (acqui/ei.hpp) and every round is a tie: the lowest eligible index.
    template <typename Params, typename Model, typename AggregatorFunction = FirstElem>
    std::vector<int64_t> believer_ei_batch(const Model& model, const std::vector<Eigen::VectorXd>& candidates, int q,
        const AggregatorFunction& afun = AggregatorFunction(), bool distinct = true)
    {
        std::vector<int64_t> idx;
        std::vector<double> score, mu;
        if (candidates.empty() || q <= 0)
            return idx;
        if (model.nb_samples() < 1) {
            for (int t = 0; t < q && (!distinct || t < (int)candidates.size()); ++t)
                idx.push_back(distinct ? t : 0);
            return idx;
        }
        Eigen::MatrixXd ms;
        Eigen::VectorXd s2;
        model.query_batch(model.samples(), ms, s2);
        double best = -std::numeric_limits<double>::infinity();
        for (int i = 0; i < (int)ms.rows(); ++i) {
            Eigen::VectorXd row(ms.cols());
            for (int p = 0; p < (int)ms.cols(); ++p)
                row(p) = ms(i, p);
            best = std::max(best, (double)afun(row));
        }
        double shift = 0.0; // a constant mean is taken off the offset instead of being added to every candidate
        batch_select_detail::means(model, candidates, afun, mu, shift);
        const double noise = model.kernel_function().noise();
        const int rc = model.select_batch(candidates, q, GPE_SELECT_EI, best + Params::acqui_ei::jitter() - shift, mu, noise, noise, distinct, idx,
            score);
        if (rc > 0)
            idx.resize((size_t)(rc - 1));
        return idx;
    }
} // namespace limbo_amd
#endif
