// limbo/experimental/acqui/eci.hpp — expected constrained improvement  ECI = P(c >= 1) EI  with the reference's semantics
// (contract: src/limbo/experimental/acqui/eci.hpp:76-130: f+ = best predicted aggregated mean over ALL training samples, feasible or
// not, cached per nb_samples; the constraint is afun(mu_c) >= 1; sigma = sqrt(sigma^2 as query() reports it); 0 when the objective's
// sigma < 1e-10 or the objective model has no sample; P = 1 when the constraint's sigma < 1e-10 or its model has no sample; no
// gradient) plus batch().  The value is exp(logcei) of include/gpe_cei.h, so it does NOT return 0 where the reference's
// X Phi(Z) + sigma phi(Z) has underflowed or cancelled: down to exp(-745) it is the correctly rounded product.  For a search use
// acqui::LogCEI (acqui/cei.hpp): the logarithm itself, with gradients.
// Interface attribution: the template signature / policy shape of this header reproduces, by requirement (drop-in for user code),
// the public interface of resibots/limbo (Copyright Inria, 2015-; CeCILL-C licence, http://www.cecill.info), file named above.
// The implementation behind the interface is this project's own.
#ifndef LIMBO_EXPERIMENTAL_ACQUI_ECI_HPP
#define LIMBO_EXPERIMENTAL_ACQUI_ECI_HPP
#include <algorithm>
#include <cmath>
#include <limits>
#include <stdexcept>
#include <vector>

#include <Eigen/Core>

#include <limbo/acqui/cei.hpp>
#include <limbo/opt/optimizer.hpp>
#include <limbo/tools/macros.hpp>

namespace limbo {
    namespace defaults {
        struct acqui_eci {
            BO_PARAM(double, jitter, 0.0);
        };
    } // namespace defaults
    namespace experimental {
        namespace acqui {
            template <typename Params, typename Model, typename ConstraintModel>
            class ECI {
            public:
                ECI(const Model& model, const ConstraintModel& constraint_model, int /*iteration*/ = 0)
                    : _model(model), _constraint_model(constraint_model), _nb_samples(-1), _f_max(0) {}
                size_t dim_in() const { return _model.dim_in(); }
                size_t dim_out() const { return _model.dim_out(); }

                template <typename AggregatorFunction>
                opt::eval_t operator()(const Eigen::VectorXd& v, const AggregatorFunction& afun, bool gradient)
                {
                    if (gradient)
                        throw std::logic_error("limbo_amd: experimental::acqui::ECI has no gradient (as the reference); acqui::LogCEI has");
                    return opt::no_grad(batch(std::vector<Eigen::VectorXd>(1, v), afun)[0]);
                }

                /// the value at every point: one query_batch per model, then the kernel of include/gpe_cei.h on the beliefs
                template <typename AggregatorFunction>
                std::vector<double> batch(const std::vector<Eigen::VectorXd>& points, const AggregatorFunction& afun)
                {
                    const size_t M = points.size();
                    std::vector<double> out(M, 0.0);
                    if (M == 0 || _model.samples().size() < 1)
                        return out;
                    _refresh(afun);
                    Eigen::MatrixXd mu, cmu;
                    Eigen::VectorXd s2, cs2;
                    _model.query_batch(points, mu, s2);
                    _constraint_model.query_batch(points, cmu, cs2);
                    const bool no_constraint_data = _constraint_model.samples().size() < 1;
                    const std::vector<double> thr(1, 1.0);
                    std::vector<double> mu0(M), s0(M), mu_c(M), s_c(M), v;
                    for (size_t m = 0; m < M; ++m) {
                        mu0[m] = afun(limbo_amd::beliefs::row_of(mu, m));
                        s0[m] = std::sqrt(s2(m));
                        mu_c[m] = afun(limbo_amd::beliefs::row_of(cmu, m));
                        s_c[m] = std::sqrt(cs2(m));
                        if (s_c[m] < 1e-10 || no_constraint_data) { // the reference's P = 1: a constraint met without uncertainty
                            mu_c[m] = 1.0;
                            s_c[m] = 0.0;
                        }
                    }
                    limbo_amd::cei_detail::values(_model, &_constraint_model, true, _f_max, Params::acqui_eci::jitter(), thr, mu0, s0, mu_c, s_c, v,
                        nullptr, nullptr);
                    for (size_t m = 0; m < M; ++m)
                        out[m] = s0[m] < 1e-10 ? 0.0 : std::exp(v[m]);
                    return out;
                }

            protected:
                const Model& _model;
                const ConstraintModel& _constraint_model;
                int _nb_samples;
                double _f_max;

                // the best predicted observation so far, feasible or not (one query_batch where the reference calls mu() per sample)
                template <typename AggregatorFunction>
                void _refresh(const AggregatorFunction& afun)
                {
                    if (_nb_samples == _model.nb_samples())
                        return;
                    Eigen::MatrixXd mu;
                    Eigen::VectorXd s2;
                    _model.query_batch(_model.samples(), mu, s2);
                    double best = -std::numeric_limits<double>::infinity();
                    for (int i = 0; i < (int)mu.rows(); ++i)
                        best = std::max(best, (double)afun(limbo_amd::beliefs::row_of(mu, (size_t)i)));
                    _nb_samples = _model.nb_samples();
                    _f_max = best;
                }
            };
        } // namespace acqui
    } // namespace experimental
} // namespace limbo
#endif
