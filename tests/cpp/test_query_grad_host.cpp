// Driver of GP::query_grad_batch, acqui::UCB / EI::batch_grad and opt::BatchGradSearch on a HOST-RESIDENT model (below
// Params::gpu::min_n_for_gpu samples; tests/test_query_grad_host.py raises LIMBO_AMD_HOST_BATCH_CROSSOVER so that no batch goes to
// the device): runs without a GPU.  Protocol: query_grad_driver.hpp.
#include <limbo/tools/macros.hpp>
#include <limbo/kernel/kernel.hpp>
#include <limbo/kernel/squared_exp_ard.hpp>
#include <limbo/kernel/matern_five_halves.hpp>
#include <limbo/kernel/matern_three_halves.hpp>
#include <limbo/kernel/exp.hpp>
#include <limbo/opt/rprop.hpp>
#include <limbo/opt/batch_grad_search.hpp>
#include <limbo/acqui/ucb.hpp>
#include <limbo/acqui/ei.hpp>

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
    struct acqui_ucb : public limbo::defaults::acqui_ucb {
    };
    struct acqui_ei : public limbo::defaults::acqui_ei {
    };
    struct opt_rprop : public limbo::defaults::opt_rprop {
        BO_PARAM(int, iterations, 60);
    };
    struct opt_batchgradsearch : public limbo::defaults::opt_batchgradsearch {
        BO_PARAM(int, points, 512);
        BO_PARAM(int, starts, 8);
        BO_PARAM(int, seed, 7);
    };
    struct gpu {
        BO_PARAM(int, device, 0);
    };
};
struct ParamsSearch : public Params {
    struct acqui_ucb {
        BO_PARAM(double, alpha, 0.0);
    };
};

#include "query_grad_driver.hpp"

int main(int argc, char** argv) { return driver_main(argc, argv); }
