// Driver for the joint posterior of the drop-in model::GP (query_joint, sample, acqui/thompson.hpp).  Where the model lives is
// decided as everywhere by Params::gpu::min_n_for_gpu() / LIMBO_AMD_MIN_N_FOR_GPU: with a large value nothing touches the device
// and the driver runs on a box WITHOUT a GPU (tests/test_joint_posterior.py), with the default the larger models run on it
// (tests/test_gpu_joint_posterior.py).
//   test_joint_dropin <input file> [brief] : kind mean P D n M S q jitter seed, then n rows of X (D) and Y (P), M query points,
//                                    M S P standard normals (point fastest, then draw, then output)
// prints: mu, cov (column-major), sigma (model.sigma per point), F (point fastest, draw, output), seed_repeat (1: the same seed gave
// the same draws twice), thompson (q indices) and thompson_host (the host arg-max over sample() with the same seed); n = 0: the
// empty model (the prior).  brief: the two thompson lines only (a candidate set of thousands: cov would be megabytes of text).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <vector>

#include <limbo/acqui/thompson.hpp>
#include <limbo/kernel/matern_five_halves.hpp>
#include <limbo/kernel/squared_exp_ard.hpp>
#include <limbo/mean/constant.hpp>
#include <limbo/mean/data.hpp>
#include <limbo/model/gp.hpp>

struct Params {
    struct kernel : public limbo::defaults::kernel {
        BO_PARAM(double, noise, 0.01);
    };
    struct kernel_squared_exp_ard : public limbo::defaults::kernel_squared_exp_ard {
    };
    struct kernel_maternfivehalves : public limbo::defaults::kernel_maternfivehalves {
    };
    struct mean_constant {
        BO_PARAM(double, constant, 1.0);
    };
    struct opt_rprop : public limbo::defaults::opt_rprop {
    };
    struct gpu {
        BO_PARAM(int, device, 0);
    };
};

template <typename GP>
static void dump(const GP& gp, const std::vector<Eigen::VectorXd>& Q, const std::vector<double>& Z, int P, int M, int S, double jitter,
    unsigned long long seed)
{
    Eigen::MatrixXd mu, cov;
    gp.query_joint(Q, mu, cov, jitter);
    std::printf("mu");
    for (int p = 0; p < P; ++p)
        for (int m = 0; m < M; ++m)
            std::printf(" %.17g", mu(m, p));
    std::printf("\ncov");
    for (int b = 0; b < M; ++b)
        for (int a = 0; a < M; ++a)
            std::printf(" %.17g", cov(a, b));
    std::printf("\nsigma");
    for (int m = 0; m < M; ++m)
        std::printf(" %.17g", gp.sigma(Q[m]));
    const std::vector<Eigen::MatrixXd> F = gp.sample(Q, Z, S, jitter);
    std::printf("\nF");
    for (int p = 0; p < P; ++p)
        for (int s = 0; s < S; ++s)
            for (int m = 0; m < M; ++m)
                std::printf(" %.17g", F[(size_t)s](m, p));
    const std::vector<Eigen::MatrixXd> A = gp.sample(Q, S, seed, jitter), B = gp.sample(Q, S, seed, jitter), C = gp.sample(Q, S, seed + 1, jitter);
    bool same = true, differs = false;
    for (int s = 0; s < S; ++s)
        for (int p = 0; p < P; ++p)
            for (int m = 0; m < M; ++m) {
                same = same && A[(size_t)s](m, p) == B[(size_t)s](m, p);
                differs = differs || A[(size_t)s](m, p) != C[(size_t)s](m, p);
            }
    std::printf("\nseed_repeat %d %d\n", (int)same, (int)differs);
}

template <typename Kernel, typename Mean>
static int run(FILE* f, int P, int D, int n, int M, int S, int q, double jitter, unsigned long long seed, bool brief)
{
    std::vector<Eigen::VectorXd> X, Y, Q;
    for (int i = 0; i < n; ++i) {
        Eigen::VectorXd x(D), y(P);
        for (int d = 0; d < D; ++d)
            if (std::fscanf(f, "%lf", &x(d)) != 1)
                return 2;
        for (int p = 0; p < P; ++p)
            if (std::fscanf(f, "%lf", &y(p)) != 1)
                return 2;
        X.push_back(x);
        Y.push_back(y);
    }
    for (int m = 0; m < M; ++m) {
        Eigen::VectorXd v(D);
        for (int d = 0; d < D; ++d)
            if (std::fscanf(f, "%lf", &v(d)) != 1)
                return 2;
        Q.push_back(v);
    }
    std::vector<double> Z((size_t)M * S * P);
    for (double& z : Z)
        if (std::fscanf(f, "%lf", &z) != 1)
            return 2;
    limbo::model::GP<Params, Kernel, Mean> gp(D, P);
    if (n > 0)
        gp.compute(X, Y);
    std::printf("host_resident %d\n", (int)gp.host_resident());
    if (!brief)
        dump(gp, Q, Z, P, M, S, jitter, seed);
    const std::vector<int64_t> idx = limbo_amd::thompson_batch(gp, Q, q, limbo_amd::FirstElem(), seed, jitter);
    const std::vector<Eigen::MatrixXd> T = gp.sample(Q, q, seed, jitter);
    std::printf("thompson");
    for (int64_t i : idx)
        std::printf(" %lld", (long long)i);
    std::printf("\nthompson_host");
    for (int s = 0; s < q; ++s) {
        int best = 0;
        for (int m = 1; m < M; ++m)
            if (T[(size_t)s](m, 0) > T[(size_t)s](best, 0))
                best = m;
        std::printf(" %d", best);
    }
    std::printf("\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2)
        return 1;
    FILE* f = std::fopen(argv[1], "r");
    if (!f)
        return 1;
    const bool brief = argc > 2;
    int kind, mean, P, D, n, M, S, q;
    double jitter;
    unsigned long long seed;
    if (std::fscanf(f, "%d %d %d %d %d %d %d %d %lf %llu", &kind, &mean, &P, &D, &n, &M, &S, &q, &jitter, &seed) != 10)
        return 2;
    using namespace limbo;
    if (kind == 0 && mean == 0)
        return run<kernel::SquaredExpARD<Params>, mean::Data<Params>>(f, P, D, n, M, S, q, jitter, seed, brief);
    if (kind == 0 && mean == 2)
        return run<kernel::SquaredExpARD<Params>, mean::Constant<Params>>(f, P, D, n, M, S, q, jitter, seed, brief);
    if (kind == 1 && mean == 0)
        return run<kernel::MaternFiveHalves<Params>, mean::Data<Params>>(f, P, D, n, M, S, q, jitter, seed, brief);
    if (kind == 1 && mean == 2)
        return run<kernel::MaternFiveHalves<Params>, mean::Constant<Params>>(f, P, D, n, M, S, q, jitter, seed, brief);
    return 3;
}
