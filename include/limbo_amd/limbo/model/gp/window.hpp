// window.hpp — a model that forgets: add a sample, then drop the oldest beyond a fixed window (an addition; the reference has no
// removal).  Works with model::GP and model::MultiGP: anything with add_sample, remove_samples and nb_samples.
#ifndef LIMBO_MODEL_GP_WINDOW_HPP
#define LIMBO_MODEL_GP_WINDOW_HPP

#include <cstddef>
#include <numeric>
#include <vector>

#include <Eigen/Core>

namespace limbo_amd {
    /// gp.add_sample(x, y), then the oldest samples beyond max_samples leave in ONE remove_samples call (one update of the
    /// factor: include/gpe_remove.h).  max_samples == 0 keeps everything.
    template <typename GP>
    void add_sample_windowed(GP& gp, const Eigen::VectorXd& x, const Eigen::VectorXd& y, size_t max_samples)
    {
        gp.add_sample(x, y);
        const size_t n = (size_t)gp.nb_samples();
        if (max_samples == 0 || n <= max_samples)
            return;
        std::vector<size_t> oldest(n - max_samples);
        std::iota(oldest.begin(), oldest.end(), (size_t)0);
        gp.remove_samples(oldest);
    }
} // namespace limbo_amd

#endif
