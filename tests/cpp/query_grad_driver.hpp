// Shared body of the two drivers of GP::query_grad_batch, acqui::UCB / EI::batch_grad and opt::BatchGradSearch
// (test_query_grad_host.cpp: a host-resident model, runs without a GPU; test_query_grad_dropin.cpp: on the device).  Where the
// model lives is decided as everywhere by Params::gpu::min_n_for_gpu() / LIMBO_AMD_MIN_N_FOR_GPU and
// LIMBO_AMD_HOST_BATCH_CROSSOVER.  The including file defines `Params` (acqui_ucb::alpha 0.5) and `ParamsSearch` (alpha 0) first.
//   <driver> grad <file>   : kind P D n M nk, nk log-parameters, n rows of X (D) and Y (P), M points
//       prints host_resident, mu (m fastest, then p), s2, dmu (m fastest, then d, then p), ds2 (m fastest, then d), ucb, ducb, ei, dei
//       (values per point; gradients m fastest, then d), one (operator() with gradient on point 0: UCB value, gradient, then EI's)
//       and same_bits (1: operator() without gradient gives UCB's value as formed from query(), bit for bit, and no gradient)
//   <driver> search <file> : D n bins, n rows of X (D) and y; a Matern-5/2 GP, UCB with alpha = 0 (the posterior mean)
//       prints grid_best (the best value of the (bins + 1)^D grid through batch()), search_value (batch() at BatchGradSearch's point)
//       and search_point
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <limbo/acqui/ei.hpp>
#include <limbo/acqui/ucb.hpp>
#include <limbo/kernel/exp.hpp>
#include <limbo/kernel/matern_five_halves.hpp>
#include <limbo/kernel/matern_three_halves.hpp>
#include <limbo/kernel/squared_exp_ard.hpp>
#include <limbo/mean/constant.hpp>
#include <limbo/model/gp.hpp>
#include <limbo/opt/batch_grad_search.hpp>

static bool read_rows(FILE* f, int rows, int D, int P, std::vector<Eigen::VectorXd>& X, std::vector<Eigen::VectorXd>* Y)
{
    for (int i = 0; i < rows; ++i) {
        Eigen::VectorXd x(D), y(P);
        for (int d = 0; d < D; ++d)
            if (std::fscanf(f, "%lf", &x(d)) != 1)
                return false;
        for (int p = 0; p < P && Y; ++p)
            if (std::fscanf(f, "%lf", &y(p)) != 1)
                return false;
        X.push_back(x);
        if (Y)
            Y->push_back(y);
    }
    return true;
}
static void print_vec(const char* name, const std::vector<double>& v)
{
    std::printf("%s", name);
    for (double x : v)
        std::printf(" %.17g", x);
    std::printf("\n");
}
static void flatten(const std::vector<Eigen::VectorXd>& g, int D, std::vector<double>& out)
{
    out.clear();
    for (int d = 0; d < D; ++d)
        for (size_t m = 0; m < g.size(); ++m)
            out.push_back(g[m](d));
}

template <typename Kernel>
static int run_grad(FILE* f, int P, int D, int n, int M, int nk)
{
    using GP_t = limbo::model::GP<Params, Kernel, limbo::mean::Constant<Params>>;
    Eigen::VectorXd th(nk);
    for (int q = 0; q < nk; ++q)
        if (std::fscanf(f, "%lf", &th(q)) != 1)
            return 2;
    std::vector<Eigen::VectorXd> X, Y, Q;
    if (!read_rows(f, n, D, P, X, &Y) || !read_rows(f, M, D, 0, Q, nullptr))
        return 2;
    GP_t gp(D, P);
    gp.kernel_function().set_h_params(th);
    gp.compute(X, Y);
    std::printf("host_resident %d\n", (int)gp.host_resident());
    Eigen::MatrixXd mu, ds2;
    Eigen::VectorXd s2;
    std::vector<Eigen::MatrixXd> dmu;
    gp.query_grad_batch(Q, mu, s2, dmu, ds2);
    Eigen::MatrixXd mu0;
    Eigen::VectorXd s20;
    gp.query_batch(Q, mu0, s20);
    std::vector<double> o;
    for (int p = 0; p < P; ++p)
        for (int m = 0; m < M; ++m)
            o.push_back(mu(m, p));
    print_vec("mu", o);
    o.clear();
    for (int m = 0; m < M; ++m)
        o.push_back(s2(m));
    print_vec("s2", o);
    o.clear();
    for (int p = 0; p < P; ++p)
        for (int d = 0; d < D; ++d)
            for (int m = 0; m < M; ++m)
                o.push_back(dmu[(size_t)m](p, d));
    print_vec("dmu", o);
    o.clear();
    for (int d = 0; d < D; ++d)
        for (int m = 0; m < M; ++m)
            o.push_back(ds2(m, d));
    print_vec("ds2", o);
    // the value outputs against query_batch's own (the same routing on either side of the crossover: to rounding)
    double dq = 0.0;
    for (int m = 0; m < M; ++m) {
        dq = std::max(dq, std::fabs(s2(m) - s20(m)));
        for (int p = 0; p < P; ++p)
            dq = std::max(dq, std::fabs(mu(m, p) - mu0(m, p)));
    }
    std::printf("vs_query_batch %.17g\n", dq);
    limbo_amd::FirstElem afun;
    limbo::acqui::UCB<Params, GP_t> ucb(gp);
    limbo::acqui::EI<Params, GP_t> ei(gp);
    std::vector<double> val;
    std::vector<Eigen::VectorXd> gr;
    ucb.batch_grad(Q, afun, val, gr);
    print_vec("ucb", val);
    flatten(gr, D, o);
    print_vec("ducb", o);
    ei.batch_grad(Q, afun, val, gr);
    print_vec("ei", val);
    flatten(gr, D, o);
    print_vec("dei", o);
    // operator(): with the gradient through the same code for one point; without it unchanged
    const limbo::opt::eval_t u1 = ucb(Q[0], afun, true), e1 = ei(Q[0], afun, true);
    o.clear();
    o.push_back(limbo::opt::fun(u1));
    for (int d = 0; d < D; ++d)
        o.push_back(limbo::opt::grad(u1)(d));
    o.push_back(limbo::opt::fun(e1));
    for (int d = 0; d < D; ++d)
        o.push_back(limbo::opt::grad(e1)(d));
    print_vec("one", o);
    bool same = true;
    for (int m = 0; m < M; ++m) {
        Eigen::VectorXd mq;
        double sq;
        std::tie(mq, sq) = gp.query(Q[m]); // the functor's value as it has always been formed (acqui/ucb.hpp)
        const limbo::opt::eval_t u0 = ucb(Q[m], afun, false);
        same = same && limbo::opt::fun(u0) == afun(mq) + Params::acqui_ucb::alpha() * std::sqrt(sq) && !u0.second.is_initialized();
        same = same && !ei(Q[m], afun, false).second.is_initialized();
    }
    std::printf("same_bits %d\n", (int)same);
    return 0;
}

static int run_search(FILE* f)
{
    using Kernel = limbo::kernel::MaternFiveHalves<ParamsSearch>;
    using GP_t = limbo::model::GP<ParamsSearch, Kernel, limbo::mean::Constant<ParamsSearch>>;
    int D, n, bins;
    if (std::fscanf(f, "%d %d %d", &D, &n, &bins) != 3)
        return 2;
    std::vector<Eigen::VectorXd> X, Y;
    if (!read_rows(f, n, D, 1, X, &Y))
        return 2;
    GP_t gp(D, 1);
    gp.compute(X, Y);
    std::printf("host_resident %d\n", (int)gp.host_resident());
    limbo_amd::FirstElem afun;
    limbo::acqui::UCB<ParamsSearch, GP_t> ucb(gp);
    // the grid, dimension 0 slowest
    size_t total = 1;
    for (int d = 0; d < D; ++d)
        total *= (size_t)(bins + 1);
    std::vector<Eigen::VectorXd> pts(total, Eigen::VectorXd(D));
    for (size_t i = 0; i < total; ++i) {
        size_t r = i;
        for (int d = D; d-- > 0;) {
            pts[i](d) = (double)(r % (size_t)(bins + 1)) / bins;
            r /= (size_t)(bins + 1);
        }
    }
    const std::vector<double> v = ucb.batch(pts, afun);
    double best = v[0];
    for (double x : v)
        best = std::max(best, x);
    auto obj = limbo::opt::make_batch_objective(ucb, afun);
    const Eigen::VectorXd x = limbo::opt::BatchGradSearch<ParamsSearch>()(obj, Eigen::VectorXd::Constant(D, 0.5), true);
    const double sv = ucb.batch(std::vector<Eigen::VectorXd>(1, x), afun)[0];
    std::printf("grid_best %.17g\nsearch_value %.17g\nsearch_point", best, sv);
    for (int d = 0; d < D; ++d)
        std::printf(" %.17g", x(d));
    std::printf("\n");
    return 0;
}

static int driver_main(int argc, char** argv)
{
    if (argc < 3)
        return 1;
    FILE* f = std::fopen(argv[2], "r");
    if (!f)
        return 1;
    if (!std::strcmp(argv[1], "search"))
        return run_search(f);
    int kind, P, D, n, M, nk;
    if (std::fscanf(f, "%d %d %d %d %d %d", &kind, &P, &D, &n, &M, &nk) != 6)
        return 2;
    using namespace limbo;
    if (kind == 0)
        return run_grad<kernel::SquaredExpARD<Params>>(f, P, D, n, M, nk);
    if (kind == 1)
        return run_grad<kernel::MaternFiveHalves<Params>>(f, P, D, n, M, nk);
    if (kind == 2)
        return run_grad<kernel::MaternThreeHalves<Params>>(f, P, D, n, M, nk);
    if (kind == 3)
        return run_grad<kernel::Exp<Params>>(f, P, D, n, M, nk);
    return 3;
}
