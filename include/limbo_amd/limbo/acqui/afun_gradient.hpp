// limbo/acqui/afun_gradient.hpp — d afun / d mu for the acquisition functors' gradients (an addition; not in limbo).
// limbo's aggregators map the dim_out predicted means to one number and say nothing about derivatives.  Two cases are served:
// limbo_amd::FirstElem (bo_base.hpp's default: the first output, derivative e_0) and any aggregator with a member
// gradient(mu) -> Eigen::VectorXd.  Anything else does not compile, with a message that says what is missing.
#ifndef LIMBO_AMD_ACQUI_AFUN_GRADIENT_HPP
#define LIMBO_AMD_ACQUI_AFUN_GRADIENT_HPP
#include <type_traits>
#include <utility>

#include <Eigen/Core>
#include <limbo/acqui/thompson.hpp> // limbo_amd::FirstElem

namespace limbo_amd {
    template <typename A, typename = void>
    struct afun_has_gradient : std::false_type {};
    template <typename A>
    struct afun_has_gradient<A, decltype((void)std::declval<const A&>().gradient(std::declval<const Eigen::VectorXd&>()))> : std::true_type {};

    /// can afun_gradient() be formed for this aggregator?
    template <typename A>
    struct afun_differentiable : std::integral_constant<bool, std::is_same<A, FirstElem>::value || afun_has_gradient<A>::value> {};

    inline Eigen::VectorXd afun_gradient(const FirstElem&, const Eigen::VectorXd& mu)
    {
        Eigen::VectorXd g = Eigen::VectorXd::Zero(mu.size());
        g(0) = 1.0;
        return g;
    }
    template <typename A>
    Eigen::VectorXd afun_gradient(const A& afun, const Eigen::VectorXd& mu)
    {
        static_assert(afun_has_gradient<A>::value,
            "limbo_amd: the gradient of an acquisition function needs d afun / d mu: use limbo_amd::FirstElem as the aggregator, or give the "
            "aggregator a member `Eigen::VectorXd gradient(const Eigen::VectorXd& mu) const`");
        return afun.gradient(mu);
    }
} // namespace limbo_amd
#endif
