// Driver for greedy batch selection through the drop-in model::GP (select_batch, acqui/batch_select.hpp).  Where the model lives is
// decided as everywhere by Params::gpu::min_n_for_gpu() / LIMBO_AMD_MIN_N_FOR_GPU: with a large value nothing touches the device
// and the driver runs on a box WITHOUT a GPU (tests/test_batch_select.py), with the default the larger models run on it
// (tests/test_gpu_batch_select.py).
//   test_batch_select_dropin <input file> : kind mean P D n M q agg loop, then n rows of X (D) and Y (P), M candidates (D) and, loop = 1,
//                                           M rows of observations at the candidates (P)
//   agg 0: the FirstElem aggregator, 1: the second output
// prints: host_resident; bucb / ei (the helpers' indices); ucb_argmax / ei_argmax (the arg-max of acqui::UCB::batch / acqui::EI::batch);
// ucb_idx, ucb_score, ei_idx, ei_score (select_batch with the complete means of one query_batch, and f+ as acqui::EI forms it),
// var_idx, var_score (the variance rule, no means); loop = 1: bucb2, the helper's indices after add_samples() of the first batch.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <limits>
#include <vector>

#include <limbo/acqui/batch_select.hpp>
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
    struct acqui_ucb {
        BO_PARAM(double, alpha, 2.0);
    };
    struct acqui_ei {
        BO_PARAM(double, jitter, 0.0);
    };
    struct opt_rprop : public limbo::defaults::opt_rprop {
    };
    struct gpu {
        BO_PARAM(int, device, 0);
    };
};

struct SecondElem {
    typedef double result_type;
    double operator()(const Eigen::VectorXd& x) const { return x(1); }
};

static void print_idx(const char* name, const std::vector<int64_t>& v)
{
    std::printf("%s", name);
    for (int64_t i : v)
        std::printf(" %lld", (long long)i);
    std::printf("\n");
}
static void print_val(const char* name, const std::vector<double>& v)
{
    std::printf("%s", name);
    for (double x : v)
        std::printf(" %.17g", x);
    std::printf("\n");
}
static int64_t argmax(const std::vector<double>& v)
{
    int64_t b = 0;
    for (size_t m = 1; m < v.size(); ++m)
        if (v[m] > v[(size_t)b])
            b = (int64_t)m;
    return b;
}

template <typename GP, typename Afun>
static void report(GP& gp, const std::vector<Eigen::VectorXd>& Q, const std::vector<Eigen::VectorXd>& Yq, int q, const Afun& afun, bool loop)
{
    std::printf("host_resident %d\n", (int)gp.host_resident());
    const std::vector<int64_t> b1 = limbo_amd::bucb_batch<Params>(gp, Q, q, afun), e1 = limbo_amd::believer_ei_batch<Params>(gp, Q, q, afun);
    print_idx("bucb", b1);
    print_idx("ei", e1);
    limbo::acqui::UCB<Params, GP> ucb(gp);
    limbo::acqui::EI<Params, GP> ei(gp);
    print_idx("ucb_argmax", std::vector<int64_t>(1, argmax(ucb.batch(Q, afun))));
    print_idx("ei_argmax", std::vector<int64_t>(1, argmax(ei.batch(Q, afun))));
    // the complete means, as the semantics state them
    Eigen::MatrixXd m;
    Eigen::VectorXd s2;
    gp.query_batch(Q, m, s2);
    std::vector<double> mu(Q.size());
    for (size_t i = 0; i < Q.size(); ++i) {
        Eigen::VectorXd row(m.cols());
        for (int p = 0; p < (int)m.cols(); ++p)
            row(p) = m(i, p);
        mu[i] = afun(row);
    }
    double best = 0.0;
    if (gp.nb_samples() > 0) {
        best = -std::numeric_limits<double>::infinity();
        gp.query_batch(gp.samples(), m, s2);
        for (int i = 0; i < (int)m.rows(); ++i) {
            Eigen::VectorXd row(m.cols());
            for (int p = 0; p < (int)m.cols(); ++p)
                row(p) = m(i, p);
            best = std::max(best, (double)afun(row));
        }
    }
    const double noise = gp.kernel_function().noise();
    std::vector<int64_t> idx;
    std::vector<double> score;
    gp.select_batch(Q, q, GPE_SELECT_UCB, Params::acqui_ucb::alpha(), mu, noise, noise, true, idx, score);
    print_idx("ucb_idx", idx);
    print_val("ucb_score", score);
    gp.select_batch(Q, q, GPE_SELECT_EI, best + Params::acqui_ei::jitter(), mu, noise, noise, true, idx, score);
    print_idx("ei_idx", idx);
    print_val("ei_score", score);
    gp.select_batch(Q, q, GPE_SELECT_VAR, 0.0, std::vector<double>(), 0.0, noise, false, idx, score);
    print_idx("var_idx", idx);
    print_val("var_score", score);
    if (loop) {
        std::vector<Eigen::VectorXd> xs, ys;
        for (int64_t i : b1) {
            xs.push_back(Q[(size_t)i]);
            ys.push_back(Yq[(size_t)i]);
        }
        gp.add_samples(xs, ys);
        print_idx("bucb2", limbo_amd::bucb_batch<Params>(gp, Q, q, afun));
    }
}

template <typename Kernel, typename Mean>
static int run(FILE* f, int P, int D, int n, int M, int q, int agg, int loop)
{
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
    std::vector<Eigen::VectorXd> XY, X, Y, Q, Yq;
    if (!rows(n, D + P, XY) || !rows(M, D, Q) || (loop && !rows(M, P, Yq)))
        return 2;
    for (const auto& r : XY) {
        Eigen::VectorXd x(D), y(P);
        for (int d = 0; d < D; ++d)
            x(d) = r(d);
        for (int p = 0; p < P; ++p)
            y(p) = r(D + p);
        X.push_back(x);
        Y.push_back(y);
    }
    limbo::model::GP<Params, Kernel, Mean> gp(D, P);
    if (n > 0)
        gp.compute(X, Y);
    if (agg == 1)
        report(gp, Q, Yq, q, SecondElem(), loop != 0);
    else
        report(gp, Q, Yq, q, limbo_amd::FirstElem(), loop != 0);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2)
        return 1;
    FILE* f = std::fopen(argv[1], "r");
    if (!f)
        return 1;
    int kind, mean, P, D, n, M, q, agg, loop;
    if (std::fscanf(f, "%d %d %d %d %d %d %d %d %d", &kind, &mean, &P, &D, &n, &M, &q, &agg, &loop) != 9)
        return 2;
    using namespace limbo;
    if (kind == 0 && mean == 0)
        return run<kernel::SquaredExpARD<Params>, mean::Data<Params>>(f, P, D, n, M, q, agg, loop);
    if (kind == 0 && mean == 2)
        return run<kernel::SquaredExpARD<Params>, mean::Constant<Params>>(f, P, D, n, M, q, agg, loop);
    if (kind == 1 && mean == 0)
        return run<kernel::MaternFiveHalves<Params>, mean::Data<Params>>(f, P, D, n, M, q, agg, loop);
    if (kind == 1 && mean == 2)
        return run<kernel::MaternFiveHalves<Params>, mean::Constant<Params>>(f, P, D, n, M, q, agg, loop);
    return 3;
}
