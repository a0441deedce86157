// Driver for the fit of the drop-in limbo::model::SPGP by the analytic gradient (include/gpe_sparse_grad.h); needs a GPU
// (tests/test_gpu_sparse_grad.py compiles and runs it).
//   test_spgp_grad <case file> : N M D, then X (N x D) row-major, y (N), log_b (D) log_c log_sig — the hyper-parameters the fit starts from
// Two models from the same seed, that is the same random subset of X as initial pseudo-inputs (M = 10 % of N):
//   default Params                   : optimize_hyperparams() does not raise the nlml, the pseudo-inputs ARE the subset, bit for bit;
//   optimize_pseudo_inputs() == true : the nlml after the fit is <= the nlml at the start, the number of pseudo-inputs is unchanged,
//                                      at least one has moved, predictions are finite with s2 > 0.
// The nlml at the start is that of a pinned model at the subset and the starting hyper-parameters.  Prints "ALL OK" and returns 0,
// or says what failed and returns 1.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <numeric>
#include <random>
#include <vector>

#include <limbo/experimental/model/spgp.hpp>
#include <limbo/kernel/squared_exp_ard.hpp>
#include <limbo/mean/null_function.hpp>

struct Params {
    struct kernel : public limbo::defaults::kernel {
    };
    struct kernel_squared_exp_ard : public limbo::defaults::kernel_squared_exp_ard {
    };
    struct model_spgp : public limbo::defaults::model_spgp {
    };
    struct opt_rprop : public limbo::defaults::opt_rprop {
        BO_PARAM(int, iterations, 40);
    };
    struct gpu {
        BO_PARAM(int, device, 0);
    };
};
struct ParamsXb : public Params {
    struct model_spgp : public limbo::defaults::model_spgp {
        BO_PARAM(bool, optimize_pseudo_inputs, true);
    };
};
template <typename P> using SPGP_of = limbo::model::SPGP<P, limbo::kernel::SquaredExpARD<P>, limbo::mean::NullFunction<P>>;

static int fails = 0;
#define CHECK(cond, ...)                   \
    do {                                   \
        if (!(cond)) {                     \
            ++fails;                       \
            std::printf("FAILED: " __VA_ARGS__); \
            std::printf("\n");             \
        }                                  \
    } while (0)

static const unsigned long long SEED = 11;

int main(int argc, char** argv)
{
    if (argc < 2)
        return 2;
    std::ifstream in(argv[1]);
    int N, M, D;
    in >> N >> M >> D;
    Eigen::MatrixXd X(N, D), Y(N, 1);
    for (int i = 0; i < N; ++i)
        for (int d = 0; d < D; ++d)
            in >> X(i, d);
    for (int i = 0; i < N; ++i)
        in >> Y(i, 0);
    Eigen::VectorXd log_b(D);
    double log_c, log_sig;
    for (int d = 0; d < D; ++d)
        in >> log_b(d);
    in >> log_c >> log_sig;
    if (!in) {
        std::printf("FAILED: short case file\n");
        return 1;
    }
    std::vector<Eigen::VectorXd> xs, ys;
    for (int i = 0; i < N; ++i) {
        Eigen::VectorXd x(D), y(1);
        for (int d = 0; d < D; ++d)
            x(d) = X(i, d);
        y(0) = Y(i, 0);
        xs.push_back(x);
        ys.push_back(y);
    }
    // the subset the models choose (spgp.hpp:417-421 as the drop-in does it: a std::mt19937, std::shuffle)
    std::mt19937 rng;
    rng.seed(SEED);
    std::vector<int> pos((size_t)N);
    std::iota(pos.begin(), pos.end(), 0);
    std::shuffle(pos.begin(), pos.end(), rng);
    Eigen::MatrixXd subset(M, D);
    for (int j = 0; j < M; ++j)
        for (int d = 0; d < D; ++d)
            subset(j, d) = X(pos[(size_t)j], d);
    Eigen::MatrixXd Xt(16, D);
    for (int i = 0; i < 16; ++i)
        for (int d = 0; d < D; ++d)
            Xt(i, d) = 0.05 + 0.9 * std::fmod(0.37 * (i + 1) * (d + 1), 1.0);

    // the start: a pinned model
    SPGP_of<Params> start(D, 1);
    start.set_pseudo_samples(subset);
    start.set_h_params(log_b, log_c, log_sig);
    start.compute(X, Y);
    CHECK(start.status() == 0, "start: status %d", start.status());
    const double nlml0 = start.nlml()(0);

    // 1. default Params: the D + 2 log-parameters only
    {
        SPGP_of<Params> gp(xs, ys);
        gp.set_seed(SEED);
        gp.set_h_params(log_b, log_c, log_sig);
        gp.optimize_hyperparams();
        const double nlml1 = gp.nlml()(0);
        std::printf("default: nlml %.6f -> %.6f\n", nlml0, nlml1);
        CHECK(nlml1 <= nlml0, "default: nlml rose: %.12f -> %.12f", nlml0, nlml1);
        CHECK(gp.nb_pseudo_samples() == M, "default: %d pseudo-inputs", gp.nb_pseudo_samples());
        const std::vector<Eigen::VectorXd> xb = gp.pseudo_samples();
        int moved = 0;
        for (int j = 0; j < M && (int)xb.size() == M; ++j)
            for (int d = 0; d < D; ++d)
                moved += xb[(size_t)j](d) != subset(j, d);
        CHECK(moved == 0, "default: %d coordinates of the pseudo-inputs differ from the subset", moved);
    }
    // 2. opt-in: the pseudo-inputs are parameters too
    {
        SPGP_of<ParamsXb> gp(xs, ys);
        gp.set_seed(SEED);
        gp.set_h_params(log_b, log_c, log_sig);
        gp.optimize_hyperparams();
        const double nlml1 = gp.nlml()(0);
        CHECK(gp.nb_pseudo_samples() == M, "opt-in: %d pseudo-inputs", gp.nb_pseudo_samples());
        const std::vector<Eigen::VectorXd> xb = gp.pseudo_samples();
        int moved = 0;
        double far = 0.0;
        for (int j = 0; j < M && (int)xb.size() == M; ++j)
            for (int d = 0; d < D; ++d) {
                moved += xb[(size_t)j](d) != subset(j, d);
                far = std::max(far, std::fabs(xb[(size_t)j](d) - subset(j, d)));
            }
        std::printf("opt-in: nlml %.6f -> %.6f, %d coordinates moved, the farthest by %.4f\n", nlml0, nlml1, moved, far);
        CHECK(nlml1 <= nlml0, "opt-in: nlml rose: %.12f -> %.12f", nlml0, nlml1);
        CHECK(moved > 0, "opt-in: no pseudo-input has moved");
        auto pr = gp.predict(Xt);
        for (int i = 0; i < 16; ++i)
            CHECK(std::isfinite(pr.first(i, 0)) && std::isfinite(pr.second(i, 0)) && pr.second(i, 0) > 0.0, "opt-in: prediction %d: %g %g", i,
                  pr.first(i, 0), pr.second(i, 0));
    }
    if (fails == 0)
        std::printf("ALL OK\n");
    return fails == 0 ? 0 : 1;
}
