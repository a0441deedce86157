// Driver for max-value entropy search in the log domain through the drop-in (model::GP::max_value_entropy, acqui/mes.hpp).  Where the
// model lives is decided as everywhere by Params::gpu::min_n_for_gpu() / LIMBO_AMD_MIN_N_FOR_GPU: with a large value nothing touches
// the device and the driver runs on a box WITHOUT a GPU (tests/test_mes_host.py), with the default the larger models run on it
// (tests/test_gpu_mes.py).
//   test_mes_dropin <input file>: kind mean D n P M noise_id observation nh K seed search, then nh log hyper-parameters (0: the
//   functor's defaults), n rows of X (D) and Y (P), M candidates (D)
//   prints: host_resident; ystar (limbo_amd::max_value_samples: K x P column-major), ystar_again (the same seed), ystar_other (seed
//   + 1), ystar_direct (GP::sample_paths and PathSet::argmax on the same draws and points), path_at_samples (per draw and output the
//   largest path value over the model's samples alone); mu (M x P column-major) and s2 (sigma^2 as query_batch reports it: the
//   noise included); one / terms_one / part_one (GP::max_value_entropy), one_again and best_one (limbo_amd::mes_batch, mes_best),
//   best_none; val / grad (acqui::MES::batch_grad; grad row-major M x D), obj (MES through opt::make_batch_objective), single
//   (operator() of candidate 0 with its gradient), plain / plain_val / plain_grad (the same object with log_value = false), first
//   (MES of output 0 alone through outs).  search = 1: one opt::BatchGradSearch run on MES: search_mu / search_s2 (the beliefs at
//   the search's own candidates, drawn here as it draws them), search_starts_logmes, search_starts_plain, search_starts_plain_grad
//   (row-major) and search_value (logmes at the point it returns).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include <limbo/acqui/mes.hpp>
#include <limbo/kernel/matern_five_halves.hpp>
#include <limbo/kernel/squared_exp_ard.hpp>
#include <limbo/mean/data.hpp>
#include <limbo/model/gp.hpp>
#include <limbo/opt/batch_grad_search.hpp>
#include <limbo/opt/batch_search.hpp>

struct ParamsBase {
    struct kernel_squared_exp_ard : public limbo::defaults::kernel_squared_exp_ard {
    };
    struct kernel_maternfivehalves : public limbo::defaults::kernel_maternfivehalves {
    };
    struct opt_rprop : public limbo::defaults::opt_rprop {
        BO_PARAM(int, iterations, 40);
    };
    struct opt_batchgradsearch {
        BO_PARAM(int, points, 63);
        BO_PARAM(int, starts, 8);
        BO_PARAM(int, seed, 7);
    };
    struct gpu {
        BO_PARAM(int, device, 0);
    };
};
struct Params001 : public ParamsBase {
    struct kernel : public limbo::defaults::kernel {
        BO_PARAM(double, noise, 0.01);
    };
};
struct Params01 : public ParamsBase {
    struct kernel : public limbo::defaults::kernel {
        BO_PARAM(double, noise, 0.1);
    };
};

static void print_val(const char* name, const std::vector<double>& v)
{
    std::printf("%s", name);
    for (double x : v)
        std::printf(" %.17g", x);
    std::printf("\n");
}
template <typename V>
static std::vector<double> flat(const V& v)
{
    return std::vector<double>(v.data(), v.data() + v.size());
}
static std::vector<double> flat_rows(const std::vector<Eigen::VectorXd>& g)
{
    std::vector<double> out;
    for (const auto& r : g)
        for (int d = 0; d < (int)r.size(); ++d)
            out.push_back(r(d));
    return out;
}

struct Shape {
    int D, n, P, M, observation, nh, K, search;
    unsigned long long seed;
};

template <typename Params, typename Kernel, typename Mean>
static int run(FILE* f, const Shape& sh)
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
    const int P = sh.P, D = sh.D, K = sh.K;
    std::vector<Eigen::VectorXd> H, XY, X, Y, Q;
    if (!rows(sh.nh > 0 ? 1 : 0, sh.nh, H) || !rows(sh.n, D + P, XY) || !rows(sh.M, D, Q))
        return 2;
    for (const auto& r : XY) {
        X.push_back(r.head(D));
        Y.push_back(r.tail(P));
    }
    using GP = limbo::model::GP<Params, Kernel, Mean>;
    GP gp(D, P);
    if (sh.nh > 0)
        gp.kernel_function().set_h_params(H[0]);
    gp.compute(X, Y);
    std::printf("host_resident %d\n", (int)gp.host_resident());
    const bool obs = sh.observation != 0;
    const limbo_amd::FirstElem first;

    const std::vector<double> ystar = limbo_amd::max_value_samples<Params>(gp, K, sh.seed);
    print_val("ystar", ystar);
    print_val("ystar_again", limbo_amd::max_value_samples<Params>(gp, K, sh.seed));
    print_val("ystar_other", limbo_amd::max_value_samples<Params>(gp, K, sh.seed + 1));
    {
        const auto paths = gp.sample_paths(1024, K, sh.seed);
        std::vector<int64_t> idx;
        std::vector<double> fmax;
        paths.argmax(limbo_amd::mes_detail::search_points(gp, Params::opt_batchgradsearch::points(), sh.seed + 3), idx, fmax);
        print_val("ystar_direct", fmax);
        paths.argmax(gp.samples(), idx, fmax);
        print_val("path_at_samples", fmax);
    }

    std::vector<int> outs;
    for (int p = 0; p < P; ++p)
        outs.push_back(p);
    std::vector<double> one, part, terms;
    gp.max_value_entropy(Q, outs, ystar, obs, one, &terms, &part);
    print_val("one", one);
    print_val("terms_one", terms);
    print_val("part_one", part);
    print_val("one_again", limbo_amd::mes_batch<Params>(gp, Q, ystar, obs));
    std::printf("best_one %lld\n", (long long)limbo_amd::mes_best<Params>(gp, Q, ystar, obs));
    std::printf("best_none %lld\n", (long long)limbo_amd::mes_best<Params>(gp, std::vector<Eigen::VectorXd>(), ystar, obs));
    print_val("first", limbo_amd::mes_batch<Params>(gp, Q, std::vector<double>(ystar.begin(), ystar.begin() + K), obs, std::vector<int>(1, 0)));
    Eigen::MatrixXd mu;
    Eigen::VectorXd s2;
    gp.query_batch(Q, mu, s2);
    print_val("mu", flat(mu));
    print_val("s2", flat(s2));

    using Acq = limbo::acqui::MES<Params, GP>;
    Acq acq(gp, ystar, true, obs), plain(gp, ystar, false, obs);
    std::vector<double> val;
    std::vector<Eigen::VectorXd> grads;
    acq.batch_grad(Q, first, val, grads);
    print_val("val", val);
    print_val("grad", flat_rows(grads));
    print_val("obj", limbo::opt::make_batch_objective(acq, first).batch(Q));
    if (sh.M > 0) {
        const limbo::opt::eval_t e = acq(Q[0], first, true);
        std::vector<double> single(1, std::get<0>(e));
        const Eigen::VectorXd g = std::get<1>(e).get();
        for (int d = 0; d < D; ++d)
            single.push_back(g(d));
        print_val("single", single);
    }
    print_val("plain", plain.batch(Q, first));
    plain.batch_grad(Q, first, val, grads);
    print_val("plain_val", val);
    print_val("plain_grad", flat_rows(grads));
    print_val("drawn", Acq(gp, K, sh.seed, true, obs).max_values());

    if (sh.search) {
        std::mt19937_64 g((unsigned)Params::opt_batchgradsearch::seed()); // opt::BatchGradSearch's own candidates, as it draws them
        std::uniform_real_distribution<double> u01(0.0, 1.0);
        std::vector<Eigen::VectorXd> pts((size_t)Params::opt_batchgradsearch::points() + 1, Eigen::VectorXd(D));
        pts[0] = Eigen::VectorXd::Constant(D, 0.5);
        for (size_t i = 1; i < pts.size(); ++i)
            for (int d = 0; d < D; ++d)
                pts[i](d) = u01(g);
        gp.query_batch(pts, mu, s2);
        print_val("search_mu", flat(mu));
        print_val("search_s2", flat(s2));
        print_val("search_starts_logmes", acq.batch(pts, first));
        plain.batch_grad(pts, first, val, grads);
        print_val("search_starts_plain", val);
        print_val("search_starts_plain_grad", flat_rows(grads));
        auto obj = limbo::opt::make_batch_objective(acq, first);
        const Eigen::VectorXd x = limbo::opt::BatchGradSearch<Params>()(obj, pts[0], true);
        print_val("search_x", flat(x));
        print_val("search_value", acq.batch(std::vector<Eigen::VectorXd>(1, x), first));
    }
    return 0;
}

template <typename Params>
static int dispatch(FILE* f, int kind, int mean, const Shape& sh)
{
    using namespace limbo;
    if (kind == 0 && mean == 0)
        return run<Params, kernel::SquaredExpARD<Params>, mean::Data<Params>>(f, sh);
    if (kind == 1 && mean == 0)
        return run<Params, kernel::MaternFiveHalves<Params>, mean::Data<Params>>(f, sh);
    return 3;
}

int main(int argc, char** argv)
{
    if (argc < 2)
        return 1;
    FILE* f = std::fopen(argv[1], "r");
    if (!f)
        return 1;
    int kind, mean, noise_id;
    Shape sh;
    if (std::fscanf(f, "%d %d %d %d %d %d %d %d %d %d %llu %d", &kind, &mean, &sh.D, &sh.n, &sh.P, &sh.M, &noise_id, &sh.observation, &sh.nh, &sh.K,
            &sh.seed, &sh.search)
        != 12)
        return 2;
    return noise_id == 1 ? dispatch<Params01>(f, kind, mean, sh) : dispatch<Params001>(f, kind, mean, sh);
}
