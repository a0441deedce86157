// limbo/acqui/kg.hpp — the knowledge gradient with correlated beliefs over a finite set of alternatives (Frazier, Powell, Dayanik
// 2009; model::GP::knowledge_gradient, include/gpe_kg.h).
// Not in the reference: its acquisition functors score a point from the posterior AT that point (src/limbo/acqui/ucb.hpp:77-95,
// src/limbo/acqui/ei.hpp:77-120), and EI takes its incumbent f+ from noisy observations.  The knowledge gradient of a candidate is
// the expected rise of the best posterior MEAN over the alternatives after one observation there, the observation's noise being the
// kernel's: it values what a point teaches about other points and needs no incumbent.
#ifndef LIMBO_AMD_ACQUI_KG_HPP
#define LIMBO_AMD_ACQUI_KG_HPP
#include <cstdint>
#include <vector>

#include <Eigen/Core>

#include <limbo/acqui/batch_select.hpp>
#include <limbo/acqui/beliefs.hpp>

namespace limbo_amd {
    /// kg[m] of every candidate over `alternatives`; afun(mu) is the mean that is maximised.  with_self: the candidate itself is one
    /// more alternative.  Means as batch_select_detail::means forms them: one output with the FirstElem aggregator and a constant
    /// mean needs no second pass (a constant shifts every line alike and moves nothing), otherwise one query_batch each.
    template <typename Params, typename Model, typename AggregatorFunction = FirstElem>
    std::vector<double> kg_batch(const Model& model, const std::vector<Eigen::VectorXd>& alternatives,
        const std::vector<Eigen::VectorXd>& candidates, const AggregatorFunction& afun = AggregatorFunction(), bool with_self = true)
    {
        std::vector<double> kg, mu_a, mu_c;
        if (alternatives.empty() || candidates.empty())
            return kg;
        double shift = 0.0;
        if (!batch_select_detail::means(model, alternatives, afun, mu_a, shift))
            batch_select_detail::means(model, candidates, afun, mu_c, shift);
        model.knowledge_gradient(alternatives, candidates, mu_a, mu_c, model.kernel_function().noise(), with_self, kg);
        return kg;
    }

    /// the index of the candidate with the largest knowledge gradient (the lowest one on exact ties), -1 without candidates
    template <typename Params, typename Model, typename AggregatorFunction = FirstElem>
    int64_t kg_best(const Model& model, const std::vector<Eigen::VectorXd>& alternatives, const std::vector<Eigen::VectorXd>& candidates,
        const AggregatorFunction& afun = AggregatorFunction(), bool with_self = true)
    {
        return beliefs::first_argmax(kg_batch<Params>(model, alternatives, candidates, afun, with_self));
    }
} // namespace limbo_amd
#endif
