// limbo/acqui/ei.hpp — expected improvement  EI = (mu - f+ - xi) Phi(Z) + sigma phi(Z)
// (contract: src/limbo/acqui/ei.hpp:77-120: returns 0 when sigma < 1e-10 or there is no sample;
// f+ = best predicted mean over the training samples, cached per nb_samples) plus batch() and batch_grad().
// The f+ scan, N calls of model.mu() in the reference (ei.hpp:100-103), is one query_batch here.
// Interface attribution: the template signature / policy shape of this header reproduces, by requirement (drop-in
// for user code), the public interface of resibots/limbo (Copyright Inria, 2015-; CeCILL-C licence, http://www.cecill.info),
// file named above.  The implementation behind the interface is this project's own.
#ifndef LIMBO_ACQUI_EI_HPP
#define LIMBO_ACQUI_EI_HPP
#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <tuple>
#include <vector>
#include <Eigen/Core>
#include <limbo/acqui/beliefs.hpp>
#include <limbo/opt/optimizer.hpp>
#include <limbo/tools/macros.hpp>
namespace limbo {
    namespace defaults {
        struct acqui_ei {
            BO_PARAM(double, jitter, 0.0);
        };
    } // namespace defaults
    namespace acqui {
        template <typename Params, typename Model>
        class EI {
        public:
            EI(const Model& model, int /*iteration*/ = 0) : _model(model), _nb_samples(-1), _f_max(0) {}
            size_t dim_in() const { return _model.dim_in(); }
            size_t dim_out() const { return _model.dim_out(); }

            template <typename AggregatorFunction>
            opt::eval_t operator()(const Eigen::VectorXd& v, const AggregatorFunction& afun, bool gradient)
            {
                if (gradient)
                    return limbo_amd::beliefs::one_with_gradient(*this, v, afun,
                        "limbo_amd: acqui::EI with gradient: the aggregator needs a member gradient(mu) (or use limbo_amd::FirstElem)");
                Eigen::VectorXd mu;
                double sigma_sq;
                std::tie(mu, sigma_sq) = _model.query(v);
                return opt::no_grad(_value(afun(mu), std::sqrt(sigma_sq), afun));
            }
            template <typename AggregatorFunction>
            std::vector<double> batch(const std::vector<Eigen::VectorXd>& points, const AggregatorFunction& afun)
            {
                std::vector<double> fmu, sigma, out(points.size());
                limbo_amd::beliefs::aggregated(_model, points, afun, true, fmu, sigma);
                for (size_t m = 0; m < points.size(); ++m)
                    out[m] = _value(fmu[m], sigma[m], afun);
                return out;
            }

            /// values[m] as batch(), grads[m] = Phi(Z) grad m + phi(Z) grad sigma at points[m] (m = afun(mu), sigma = sqrt(sigma^2),
            /// Z = (m - f+ - xi) / sigma), zero where EI itself is (sigma < 1e-10, no samples): one device batch.  d afun / d mu:
            /// limbo_amd::afun_gradient.  The mean functor's own derivative is not included (GP::query_grad_batch).
            template <typename AggregatorFunction>
            void batch_grad(const std::vector<Eigen::VectorXd>& points, const AggregatorFunction& afun, std::vector<double>& values,
                std::vector<Eigen::VectorXd>& grads)
            {
                std::vector<double> fmu, sigma;
                std::vector<Eigen::VectorXd> gmu;
                Eigen::MatrixXd ds2;
                limbo_amd::beliefs::aggregated_grad(_model, points, afun, true, fmu, sigma, gmu, ds2);
                values.resize(points.size());
                grads.resize(points.size());
                for (size_t m = 0; m < points.size(); ++m) {
                    values[m] = _value(fmu[m], sigma[m], afun);
                    Eigen::VectorXd g = Eigen::VectorXd::Zero(ds2.cols());
                    if (!(sigma[m] < 1e-10 || _model.samples().size() < 1)) {
                        const double Z = (fmu[m] - _f_max - Params::acqui_ei::jitter()) / sigma[m];
                        const double phi = std::exp(-0.5 * Z * Z) / std::sqrt(2.0 * M_PI);
                        const double Phi = 0.5 * std::erfc(-Z / std::sqrt(2));
                        for (int d = 0; d < (int)ds2.cols(); ++d)
                            g(d) = Phi * gmu[m](d) + phi * ds2(m, d) / (2.0 * sigma[m]);
                    }
                    grads[m] = g;
                }
            }

        protected:
            const Model& _model;
            int _nb_samples;
            double _f_max;

            template <typename AggregatorFunction>
            double _value(double fmu, double sigma, const AggregatorFunction& afun)
            {
                if (sigma < 1e-10 || _model.samples().size() < 1)
                    return 0.0;
                if (_nb_samples != _model.nb_samples()) { // best predicted observation so far
                    Eigen::MatrixXd mu;
                    Eigen::VectorXd s2;
                    _model.query_batch(_model.samples(), mu, s2);
                    double best = -std::numeric_limits<double>::infinity();
                    for (int i = 0; i < (int)mu.rows(); ++i)
                        best = std::max(best, (double)afun(limbo_amd::beliefs::row_of(mu, (size_t)i)));
                    _nb_samples = _model.nb_samples();
                    _f_max = best;
                }
                const double X = fmu - _f_max - Params::acqui_ei::jitter();
                const double Z = X / sigma;
                const double phi = std::exp(-0.5 * Z * Z) / std::sqrt(2.0 * M_PI);
                const double Phi = 0.5 * std::erfc(-Z / std::sqrt(2));
                return X * Phi + sigma * phi;
            }
        };
    } // namespace acqui
} // namespace limbo
#endif
