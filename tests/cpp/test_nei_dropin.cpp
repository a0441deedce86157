// Driver for noisy expected improvement in the log domain through the drop-in (model::GP::log_noisy_ei, acqui/nei.hpp).  Where the
// model lives is decided as everywhere by Params::gpu::min_n_for_gpu() / LIMBO_AMD_MIN_N_FOR_GPU and LIMBO_AMD_HOST_BATCH_CROSSOVER:
// with large values nothing touches the device and the driver runs on a box WITHOUT a GPU (tests/test_nei_host.py), with the defaults
// the larger models run on it (tests/test_gpu_nei.py).
//   test_nei_dropin <input file>: D n M B S seed nh s_prune, then nh log hyper-parameters (0: the functor's defaults), n rows of X (D)
//   and Y (1), M candidates (D), B baseline points (D).  SE-ARD, the Data mean, kernel noise 0.01, jitter 1e-6, xi 0.01.
//   prints: host_resident; Z (the base normals: GP::standard_normals(B S, seed), B x S column-major); one / fplus / cvar / cmean
//   (GP::log_noisy_ei), batch and best (limbo_amd::lognei_batch, lognei_best with the same seed), best_none, acq (acqui::LogNEI::batch)
//   and single (its operator() on candidate 0); singular (the status for the baseline with every point listed twice and no jitter,
//   and the sum of |lognei| it leaves); baseline_idx / baseline_idx_again (limbo_amd::nei_baseline_indices, the same seed) /
//   baseline_idx_other (seed + 1), baseline_pts (nei_baseline, row-major), mu_train (the posterior mean at the samples).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <limbo/acqui/nei.hpp>
#include <limbo/acqui/thompson.hpp>
#include <limbo/kernel/squared_exp_ard.hpp>
#include <limbo/mean/data.hpp>
#include <limbo/model/gp.hpp>

struct Params {
    struct kernel_squared_exp_ard : public limbo::defaults::kernel_squared_exp_ard {
    };
    struct kernel : public limbo::defaults::kernel {
        BO_PARAM(double, noise, 0.01);
    };
    struct gpu {
        BO_PARAM(int, device, 0);
    };
};

static void print_val(const char* name, const std::vector<double>& v)
{
    std::printf("%s", name);
    for (double x : v)
        std::printf(" %.17g", x);
    std::printf("\n");
}
static void print_idx(const char* name, const std::vector<int64_t>& v)
{
    std::printf("%s", name);
    for (int64_t x : v)
        std::printf(" %lld", (long long)x);
    std::printf("\n");
}

int main(int argc, char** argv)
{
    if (argc < 2)
        return 1;
    FILE* f = std::fopen(argv[1], "r");
    if (!f)
        return 1;
    int D, n, M, B, S, nh, s_prune;
    unsigned long long seed;
    if (std::fscanf(f, "%d %d %d %d %d %llu %d %d", &D, &n, &M, &B, &S, &seed, &nh, &s_prune) != 8)
        return 2;
    auto rows = [&](int cnt, int w, std::vector<Eigen::VectorXd>& out) {
        for (int i = 0; i < cnt; ++i) {
            Eigen::VectorXd x(w);
            for (int d = 0; d < w; ++d)
                if (std::fscanf(f, "%lf", &x(d)) != 1)
                    return false;
            out.push_back(x);
        }
        return true;
    };
    std::vector<Eigen::VectorXd> H, XY, X, Y, Q, Xb;
    if (!rows(nh > 0 ? 1 : 0, nh, H) || !rows(n, D + 1, XY) || !rows(M, D, Q) || !rows(B, D, Xb))
        return 2;
    for (const auto& r : XY) {
        X.push_back(r.head(D));
        Y.push_back(r.tail(1));
    }
    using GP = limbo::model::GP<Params, limbo::kernel::SquaredExpARD<Params>, limbo::mean::Data<Params>>;
    GP gp(D, 1);
    if (nh > 0)
        gp.kernel_function().set_h_params(H[0]);
    gp.compute(X, Y);
    std::printf("host_resident %d\n", (int)gp.host_resident());
    const double jitter = 1e-6, xi = 0.01;
    const limbo_amd::FirstElem first;

    const std::vector<double> Z = GP::standard_normals((size_t)B * (size_t)S, seed);
    print_val("Z", Z);
    std::vector<double> one, fplus, cvar, cmean;
    std::printf("status %d\n", gp.log_noisy_ei(Q, Xb, Z, 0, jitter, xi, one, &fplus, &cvar, &cmean));
    print_val("one", one);
    print_val("fplus", fplus);
    print_val("cvar", cvar);
    print_val("cmean", cmean);
    print_val("batch", limbo_amd::lognei_batch<Params>(gp, Q, Xb, S, seed, jitter, xi));
    std::printf("best %lld\n", (long long)limbo_amd::lognei_best<Params>(gp, Q, Xb, S, seed, jitter, xi));
    std::printf("best_none %lld\n", (long long)limbo_amd::lognei_best<Params>(gp, std::vector<Eigen::VectorXd>(), Xb, S, seed, jitter, xi));
    limbo::acqui::LogNEI<Params, GP> acq(gp, Xb, S, seed, jitter, xi);
    print_val("acq", acq.batch(Q, first));
    if (M > 0)
        std::printf("single %.17g\n", std::get<0>(acq(Q[0], first, false)));
    {
        std::vector<Eigen::VectorXd> twice;
        for (const auto& x : Xb) {
            twice.push_back(x);
            twice.push_back(x);
        }
        std::vector<double> z2 = GP::standard_normals(twice.size() * (size_t)S, seed), v;
        const int rc = gp.log_noisy_ei(Q, twice, z2, 0, 0.0, xi, v);
        double sum = 0.0;
        for (double x : v)
            sum += std::fabs(x);
        std::printf("singular %d %.17g\n", rc, rc > 0 ? sum : 0.0);
    }
    print_idx("baseline_idx", limbo_amd::nei_baseline_indices(gp, s_prune, seed));
    print_idx("baseline_idx_again", limbo_amd::nei_baseline_indices(gp, s_prune, seed));
    print_idx("baseline_idx_other", limbo_amd::nei_baseline_indices(gp, s_prune, seed + 1));
    {
        std::vector<double> flat;
        for (const auto& x : limbo_amd::nei_baseline(gp, s_prune, seed))
            for (int d = 0; d < D; ++d)
                flat.push_back(x(d));
        print_val("baseline_pts", flat);
    }
    Eigen::MatrixXd mu;
    Eigen::VectorXd s2;
    gp.query_batch(X, mu, s2);
    print_val("mu_train", std::vector<double>(mu.data(), mu.data() + mu.size()));
    return 0;
}
