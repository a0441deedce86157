// Shared body of the two drivers of GP::sample_paths / PathSet and limbo_amd::thompson_paths_batch (test_pathwise_host.cpp: a
// host-resident model, runs without a GPU; test_pathwise_dropin.cpp: on the device).  Where the model lives is decided as everywhere
// by Params::gpu::min_n_for_gpu() / LIMBO_AMD_MIN_N_FOR_GPU.  The including file defines `Params` first.
//   <driver> paths <file>    : kind P D n T nk R S seed, nk log-parameters, n rows of X (D) and Y (P), T points, then Omega0 (R x Dw,
//                              row-major), phase (R), W (R S P), E (n S P)
//       prints host_resident, on_device, F (t fastest, then draw, then output) and dF (t fastest, then d, draw, output) of eval_grad,
//       eval_same (1: eval() alone returns eval_grad's F, bit for bit), argmax and fmax, prior_F (the same Omega0, phase, W on a model
//       without samples), seeded_same (1: sample_paths(R, S, seed) is the explicit overload on spectral_draws(seed) and
//       standard_normals(seed + 1 / + 2)), spectral_repro (1: spectral_draws gives the same twice and another for another seed),
//       spec_omega and spec_phase (spectral_draws(kind, R, Dw, seed))
//   <driver> thompson <file> : D n q seed, n rows of X (D) and y; an SE-ARD GP
//       prints host_resident, proposals (q x D, point by point), prop_value (proposal s on path s), cand_best (the best of the
//       search's own candidates on path s)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include <limbo/acqui/thompson.hpp>
#include <limbo/kernel/exp.hpp>
#include <limbo/kernel/matern_five_halves.hpp>
#include <limbo/kernel/matern_three_halves.hpp>
#include <limbo/kernel/squared_exp_ard.hpp>
#include <limbo/mean/constant.hpp>
#include <limbo/model/gp.hpp>

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
static bool read_vec(FILE* f, size_t n, std::vector<double>& v)
{
    v.resize(n);
    for (double& x : v)
        if (std::fscanf(f, "%lf", &x) != 1)
            return false;
    return true;
}
static void print_vec(const char* name, const std::vector<double>& v)
{
    std::printf("%s", name);
    for (double x : v)
        std::printf(" %.17g", x);
    std::printf("\n");
}
// F[s](t, p) -> t fastest, then draw, then output
static std::vector<double> flat_F(const std::vector<Eigen::MatrixXd>& F, int T, int S, int P)
{
    std::vector<double> o;
    for (int p = 0; p < P; ++p)
        for (int s = 0; s < S; ++s)
            for (int t = 0; t < T; ++t)
                o.push_back(F[(size_t)s](t, p));
    return o;
}

template <typename Kernel>
static int run_paths(FILE* f, int P, int D, int n, int T, int nk, int R, int S, unsigned long long seed)
{
    using GP_t = limbo::model::GP<Params, Kernel, limbo::mean::Constant<Params>>;
    namespace pw = limbo_amd::pathwise;
    constexpr int kind = limbo_amd::device_kernel<Kernel>::kind;
    Eigen::VectorXd th(nk);
    for (int q = 0; q < nk; ++q)
        if (std::fscanf(f, "%lf", &th(q)) != 1)
            return 2;
    std::vector<Eigen::VectorXd> X, Y, Q;
    if (!read_rows(f, n, D, P, X, &Y) || !read_rows(f, T, D, 0, Q, nullptr))
        return 2;
    const int Dw = pw::freq_dim(kind, nk, D);
    std::vector<double> Om, ph, W, E;
    if (!read_vec(f, (size_t)R * Dw, Om) || !read_vec(f, (size_t)R, ph) || !read_vec(f, (size_t)R * S * P, W) || !read_vec(f, (size_t)n * S * P, E))
        return 2;
    GP_t gp(D, P);
    gp.kernel_function().set_h_params(th);
    gp.compute(X, Y);
    std::printf("host_resident %d\n", (int)gp.host_resident());
    typename GP_t::PathSet ps = gp.sample_paths(R, S, Om, ph, W, E);
    std::printf("on_device %d\n", (int)ps.on_device());
    if (ps.n_draws() != S)
        return 4;
    std::vector<Eigen::MatrixXd> F, dF;
    ps.eval_grad(Q, F, dF);
    print_vec("F", flat_F(F, T, S, P));
    std::vector<double> o;
    for (int c = 0; c < S * P; ++c)
        for (int d = 0; d < D; ++d)
            for (int t = 0; t < T; ++t)
                o.push_back(dF[(size_t)c](t, d));
    print_vec("dF", o);
    typename GP_t::PathSet moved = std::move(ps); // (move-only: the set changes hands, the source is empty)
    std::printf("eval_same %d\n", (int)(flat_F(moved.eval(Q), T, S, P) == flat_F(F, T, S, P)));
    std::vector<int64_t> idx;
    std::vector<double> fmax;
    moved.argmax(Q, idx, fmax);
    o.assign(idx.begin(), idx.end());
    print_vec("argmax", o);
    print_vec("fmax", fmax);
    {
        GP_t prior(D, P);
        prior.kernel_function().set_h_params(th);
        print_vec("prior_F", flat_F(prior.sample_paths(R, S, Om, ph, W, std::vector<double>()).eval(Q), T, S, P));
    }
    const pw::Spectral sp = pw::spectral_draws(kind, R, Dw, seed), sp2 = pw::spectral_draws(kind, R, Dw, seed), sp3 = pw::spectral_draws(kind, R, Dw, seed + 1);
    std::printf("spectral_repro %d\n", (int)(sp.Omega0 == sp2.Omega0 && sp.phase == sp2.phase && sp.Omega0 != sp3.Omega0 && sp.phase != sp3.phase));
    print_vec("spec_omega", sp.Omega0);
    print_vec("spec_phase", sp.phase);
    const auto a = gp.sample_paths(R, S, seed).eval(Q);
    const auto b = gp.sample_paths(R, S, sp.Omega0, sp.phase, GP_t::standard_normals((size_t)R * S * P, seed + 1),
                         GP_t::standard_normals((size_t)n * S * P, seed + 2))
                       .eval(Q);
    std::printf("seeded_same %d\n", (int)(flat_F(a, T, S, P) == flat_F(b, T, S, P)));
    return 0;
}

static int run_thompson(FILE* f)
{
    using Kernel = limbo::kernel::SquaredExpARD<Params>;
    using GP_t = limbo::model::GP<Params, Kernel, limbo::mean::Constant<Params>>;
    int D, n, q;
    unsigned long long seed;
    if (std::fscanf(f, "%d %d %d %llu", &D, &n, &q, &seed) != 4)
        return 2;
    std::vector<Eigen::VectorXd> X, Y;
    if (!read_rows(f, n, D, 1, X, &Y))
        return 2;
    GP_t gp(D, 1);
    gp.compute(X, Y);
    std::printf("host_resident %d\n", (int)gp.host_resident());
    const int R = 256;
    const std::vector<Eigen::VectorXd> prop = limbo_amd::thompson_paths_batch<Params>(gp, q, seed, R);
    if ((int)prop.size() != q)
        return 4;
    // the search's own candidates and paths once more: both are functions of the seed
    std::mt19937_64 g(seed + 3);
    std::uniform_real_distribution<double> u01(0.0, 1.0);
    std::vector<Eigen::VectorXd> pts((size_t)Params::opt_batchgradsearch::points(), Eigen::VectorXd(D));
    for (auto& p : pts)
        for (int d = 0; d < D; ++d)
            p(d) = u01(g);
    const auto paths = gp.sample_paths(R, q, seed);
    std::vector<int64_t> idx;
    std::vector<double> cand_best, pv, pp;
    paths.argmax(pts, idx, cand_best);
    const auto Fp = paths.eval(prop);
    for (int s = 0; s < q; ++s) {
        pv.push_back(Fp[(size_t)s](s, 0));
        for (int d = 0; d < D; ++d)
            pp.push_back(prop[(size_t)s](d));
    }
    print_vec("proposals", pp);
    print_vec("prop_value", pv);
    print_vec("cand_best", cand_best);
    return 0;
}

static int driver_main(int argc, char** argv)
{
    if (argc < 3)
        return 1;
    FILE* f = std::fopen(argv[2], "r");
    if (!f)
        return 1;
    if (!std::strcmp(argv[1], "thompson"))
        return run_thompson(f);
    int kind, P, D, n, T, nk, R, S;
    unsigned long long seed;
    if (std::fscanf(f, "%d %d %d %d %d %d %d %d %llu", &kind, &P, &D, &n, &T, &nk, &R, &S, &seed) != 9)
        return 2;
    using namespace limbo;
    if (kind == 0)
        return run_paths<kernel::SquaredExpARD<Params>>(f, P, D, n, T, nk, R, S, seed);
    if (kind == 1)
        return run_paths<kernel::MaternFiveHalves<Params>>(f, P, D, n, T, nk, R, S, seed);
    if (kind == 2)
        return run_paths<kernel::MaternThreeHalves<Params>>(f, P, D, n, T, nk, R, S, seed);
    if (kind == 3)
        return run_paths<kernel::Exp<Params>>(f, P, D, n, T, nk, R, S, seed);
    return 3;
}
