// Driver for model::GP::add_samples / MultiGP::add_samples (a batch of samples in one blocked update, include/gpe_append.h).
//   test_add_samples <input file> [device]
//   input: kind mean P D n0 n1 M, then n1 rows of X (D) and Y (P), then M query points
// Without `device` Params::gpu::min_n_for_gpu keeps every model on the host (no GPU is ever asked for); with it the
// threshold is 0 and the append runs through gpe_add_samples.  Prints, after compute() on the first n0 samples and ONE
// add_samples() of the rest ("batch"), and after the add_sample() loop on a second model ("loop"): L, alpha, log_lik, mu,
// sigma^2, the status; then "multi_batch" / "multi_loop": mu of a MultiGP (null-function mean: add_samples evaluates the mean
// per new point after ONE mean update) fed the same two ways.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <vector>

#include <limbo/kernel/exp.hpp>
#include <limbo/kernel/matern_five_halves.hpp>
#include <limbo/kernel/squared_exp_ard.hpp>
#include <limbo/mean/constant.hpp>
#include <limbo/mean/data.hpp>
#include <limbo/mean/null_function.hpp>
#include <limbo/model/gp.hpp>
#include <limbo/model/multi_gp.hpp>

static int g_min_n = 1 << 20;

struct Params {
    struct kernel : public limbo::defaults::kernel {
        BO_PARAM(double, noise, 0.01);
    };
    struct kernel_squared_exp_ard : public limbo::defaults::kernel_squared_exp_ard {
    };
    struct kernel_maternfivehalves : public limbo::defaults::kernel_maternfivehalves {
    };
    struct kernel_exp : public limbo::defaults::kernel_exp {
    };
    struct mean_constant {
        BO_PARAM(double, constant, 1.0);
    };
    struct opt_rprop : public limbo::defaults::opt_rprop {
    };
    struct gpu {
        BO_PARAM(int, device, 0);
        static int min_n_for_gpu() { return g_min_n; }
    };
};

template <typename GP>
static void dump(const char* tag, GP& gp, const std::vector<Eigen::VectorXd>& Q)
{
    const Eigen::MatrixXd& L = gp.matrixL();
    const Eigen::MatrixXd& a = gp.alpha();
    std::printf("%s n %d\nL", tag, (int)gp.nb_samples());
    for (int j = 0; j < (int)L.cols(); ++j)
        for (int i = 0; i < (int)L.rows(); ++i)
            std::printf(" %.17g", L(i, j));
    std::printf("\nalpha");
    for (int p = 0; p < (int)a.cols(); ++p)
        for (int i = 0; i < (int)a.rows(); ++i)
            std::printf(" %.17g", a(i, p));
    std::printf("\nlog_lik %.17g\nmu", gp.compute_log_lik());
    for (const auto& q : Q) {
        Eigen::VectorXd m = gp.mu(q);
        for (int p = 0; p < (int)m.size(); ++p)
            std::printf(" %.17g", m(p));
    }
    std::printf("\nsigma");
    for (const auto& q : Q)
        std::printf(" %.17g", gp.sigma(q));
    std::printf("\nstatus %d\n", gp.last_status());
}

template <typename Kernel, typename Mean>
static int run(FILE* f, int P, int D, int n0, int n1, int M)
{
    std::vector<Eigen::VectorXd> X, Y, Q;
    for (int i = 0; i < n1; ++i) {
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
        Eigen::VectorXd q(D);
        for (int d = 0; d < D; ++d)
            if (std::fscanf(f, "%lf", &q(d)) != 1)
                return 2;
        Q.push_back(q);
    }
    const std::vector<Eigen::VectorXd> X0(X.begin(), X.begin() + n0), Y0(Y.begin(), Y.begin() + n0);
    const std::vector<Eigen::VectorXd> X1(X.begin() + n0, X.end()), Y1(Y.begin() + n0, Y.end());
    {
        limbo::model::GP<Params, Kernel, Mean> gp(D, P);
        if (n0 > 0)
            gp.compute(X0, Y0);
        gp.add_samples(std::vector<Eigen::VectorXd>(), std::vector<Eigen::VectorXd>()); // nothing: nothing changes
        gp.add_samples(X1, Y1);
        dump("batch", gp, Q);
    }
    {
        limbo::model::GP<Params, Kernel, Mean> gp(D, P);
        if (n0 > 0)
            gp.compute(X0, Y0);
        for (int i = n0; i < n1; ++i)
            gp.add_sample(X[i], Y[i]);
        dump("loop", gp, Q);
    }
    using Multi = limbo::model::MultiGP<Params, limbo::model::GP, Kernel, limbo::mean::NullFunction<Params>>;
    for (int pass = 0; pass < 2; ++pass) {
        Multi mgp(D, P);
        if (g_min_n == 0 && n0 > 0)
            mgp.compute(X0, Y0);
        else
            for (int i = 0; i < n0; ++i) // (MultiGP::compute factors its members as one batched device launch: not for a host model)
                mgp.add_sample(X[i], Y[i]);
        if (pass == 0)
            mgp.add_samples(X1, Y1);
        else
            for (int i = n0; i < n1; ++i)
                mgp.add_sample(X[i], Y[i]);
        std::printf("%s", pass == 0 ? "multi_batch" : "multi_loop");
        for (const auto& q : Q) {
            Eigen::VectorXd m = mgp.mu(q);
            for (int p = 0; p < (int)m.size(); ++p)
                std::printf(" %.17g", m(p));
        }
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2)
        return 1;
    if (argc > 2 && std::strcmp(argv[2], "device") == 0)
        g_min_n = 0;
    FILE* f = std::fopen(argv[1], "r");
    if (!f)
        return 1;
    int kind, mean, P, D, n0, n1, M;
    if (std::fscanf(f, "%d %d %d %d %d %d %d", &kind, &mean, &P, &D, &n0, &n1, &M) != 7)
        return 2;
    using namespace limbo;
    int rc = 3;
    if (kind == 0 && mean == 0)
        rc = run<kernel::SquaredExpARD<Params>, mean::Data<Params>>(f, P, D, n0, n1, M);
    else if (kind == 0 && mean == 1)
        rc = run<kernel::SquaredExpARD<Params>, mean::NullFunction<Params>>(f, P, D, n0, n1, M);
    else if (kind == 1 && mean == 0)
        rc = run<kernel::MaternFiveHalves<Params>, mean::Data<Params>>(f, P, D, n0, n1, M);
    else if (kind == 1 && mean == 2)
        rc = run<kernel::MaternFiveHalves<Params>, mean::Constant<Params>>(f, P, D, n0, n1, M);
    else if (kind == 3 && mean == 0)
        rc = run<kernel::Exp<Params>, mean::Data<Params>>(f, P, D, n0, n1, M);
    else if (kind == 3 && mean == 1)
        rc = run<kernel::Exp<Params>, mean::NullFunction<Params>>(f, P, D, n0, n1, M);
    std::fclose(f);
    return rc;
}
