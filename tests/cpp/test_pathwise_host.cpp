// Driver of GP::sample_paths / PathSet and limbo_amd::thompson_paths_batch on a HOST-RESIDENT model (below
// Params::gpu::min_n_for_gpu samples): runs without a GPU.  Protocol: pathwise_driver.hpp.
#include <limbo/tools/macros.hpp>
#include <limbo/kernel/kernel.hpp>
#include <limbo/kernel/squared_exp_ard.hpp>
#include <limbo/kernel/matern_five_halves.hpp>
#include <limbo/kernel/matern_three_halves.hpp>
#include <limbo/kernel/exp.hpp>
#include <limbo/opt/rprop.hpp>
#include <limbo/opt/batch_grad_search.hpp>

struct Params {
    struct kernel : public limbo::defaults::kernel {
        BO_PARAM(double, noise, 0.01);
    };
    struct kernel_squared_exp_ard : public limbo::defaults::kernel_squared_exp_ard {
    };
    struct kernel_maternfivehalves : public limbo::defaults::kernel_maternfivehalves {
    };
    struct kernel_maternthreehalves : public limbo::defaults::kernel_maternthreehalves {
    };
    struct kernel_exp : public limbo::defaults::kernel_exp {
    };
    struct mean_constant {
        BO_PARAM(double, constant, 1.0);
    };
    struct opt_rprop : public limbo::defaults::opt_rprop {
        BO_PARAM(int, iterations, 40);
    };
    struct opt_batchgradsearch : public limbo::defaults::opt_batchgradsearch {
        BO_PARAM(int, points, 512);
        BO_PARAM(int, starts, 4);
        BO_PARAM(int, seed, 7);
    };
    struct gpu {
        BO_PARAM(int, device, 0);
    };
};

#include "pathwise_driver.hpp"

int main(int argc, char** argv) { return driver_main(argc, argv); }
