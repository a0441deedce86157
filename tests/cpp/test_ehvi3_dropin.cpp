// Driver for the three-objective expected hypervolume improvement through the drop-in (model::GP::expected_hypervolume_improvement3,
// acqui/ehvi3.hpp).  Where the models live is decided as everywhere by Params::gpu::min_n_for_gpu() / LIMBO_AMD_MIN_N_FOR_GPU: with a
// large value nothing touches the device and the driver runs on a box WITHOUT a GPU (tests/test_ehvi3_host.py), with the default the
// larger models run on it (tests/test_gpu_ehvi3.py).
//   test_ehvi3_dropin <input file> : kind mean D n K M noise_id observation nh r1 r2 r3, then nh log hyper-parameters (0: the functor's
//                                    defaults), n rows of X (D) and Y (3), K objective points (3) the front is taken from, M candidates (D)
// prints: host_resident (the three-output model, and the three one-output models); front (row-major) and hv (pareto_front3,
// hypervolume3); one / best_one (ehvi3_batch, ehvi3_best on ONE model with three outputs) with mu (M x 3 column-major) and s2
// (sigma^2 as query_batch reports it: the noise included) it worked from; three / best_three (the same on THREE one-output models)
// with mu1, s2_1 .. mu3, s2_3; val / grad (acqui::Ehvi3::batch_grad; grad row-major M x D), obj (Ehvi3 through
// opt::make_batch_objective), single (operator() of candidate 0 with its gradient: value, then D numbers), and one
// opt::BatchGradSearch run on Ehvi3: search_starts (the values at the search's own candidates, drawn here as it draws them) and
// search_value (Ehvi3 at the point it returns).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include <limbo/acqui/ehvi3.hpp>
#include <limbo/kernel/matern_five_halves.hpp>
#include <limbo/kernel/squared_exp_ard.hpp>
#include <limbo/mean/constant.hpp>
#include <limbo/mean/data.hpp>
#include <limbo/model/gp.hpp>
#include <limbo/opt/batch_grad_search.hpp>
#include <limbo/opt/batch_search.hpp>

struct ParamsBase {
    struct kernel_squared_exp_ard : public limbo::defaults::kernel_squared_exp_ard {
    };
    struct kernel_maternfivehalves : public limbo::defaults::kernel_maternfivehalves {
    };
    struct mean_constant {
        BO_PARAM(double, constant, 1.0);
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

struct Shape {
    int D, n, K, M, observation, nh;
    double r[3];
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
    std::vector<Eigen::VectorXd> H, XY, X, Y, Yk[3], Fp, Q;
    if (!rows(sh.nh > 0 ? 1 : 0, sh.nh, H) || !rows(sh.n, sh.D + 3, XY) || !rows(sh.K, 3, Fp) || !rows(sh.M, sh.D, Q))
        return 2;
    for (const auto& r : XY) {
        Eigen::VectorXd x(sh.D), y(3);
        for (int d = 0; d < sh.D; ++d)
            x(d) = r(d);
        for (int k = 0; k < 3; ++k) {
            y(k) = r(sh.D + k);
            Yk[k].push_back(Eigen::VectorXd::Constant(1, y(k)));
        }
        X.push_back(x);
        Y.push_back(y);
    }
    using GP = limbo::model::GP<Params, Kernel, Mean>;
    GP gp(sh.D, 3), g1(sh.D, 1), g2(sh.D, 1), g3(sh.D, 1);
    GP* single[3] = {&g1, &g2, &g3};
    if (sh.nh > 0)
        for (GP* g : {&gp, &g1, &g2, &g3})
            g->kernel_function().set_h_params(H[0]);
    if (sh.n > 0) {
        gp.compute(X, Y);
        for (int k = 0; k < 3; ++k)
            single[k]->compute(X, Yk[k]);
    }
    std::printf("host_resident %d %d %d %d\n", (int)gp.host_resident(), (int)g1.host_resident(), (int)g2.host_resident(), (int)g3.host_resident());
    Eigen::VectorXd ref(3);
    ref << sh.r[0], sh.r[1], sh.r[2];
    const std::vector<double> front = limbo_amd::pareto_front3(Fp, ref);
    print_val("front", front);
    std::printf("hv %.17g\n", limbo_amd::hypervolume3(front, ref));
    const bool obs = sh.observation != 0;
    const limbo_amd::FirstElem first;

    print_val("one", limbo_amd::ehvi3_batch<Params>(gp, Q, front, ref, {0, 1, 2}, obs));
    std::printf("best_one %lld\n", (long long)limbo_amd::ehvi3_best<Params>(gp, Q, front, ref, {0, 1, 2}, obs));
    std::printf("best_none %lld\n", (long long)limbo_amd::ehvi3_best<Params>(gp, std::vector<Eigen::VectorXd>(), front, ref));
    Eigen::MatrixXd mu;
    Eigen::VectorXd s2;
    gp.query_batch(Q, mu, s2);
    print_val("mu", flat(mu));
    print_val("s2", flat(s2));

    print_val("three", limbo_amd::ehvi3_batch<Params>(g1, g2, g3, Q, front, ref, first, obs));
    std::printf("best_three %lld\n", (long long)limbo_amd::ehvi3_best<Params>(g1, g2, g3, Q, front, ref, first, obs));
    const char* names[3][2] = {{"mu1", "s2_1"}, {"mu2", "s2_2"}, {"mu3", "s2_3"}};
    for (int k = 0; k < 3; ++k) {
        single[k]->query_batch(Q, mu, s2);
        print_val(names[k][0], flat(mu));
        print_val(names[k][1], flat(s2));
    }

    limbo::acqui::Ehvi3<Params, GP> acq(g1, g2, g3, front, ref, obs);
    std::vector<double> val, gr;
    std::vector<Eigen::VectorXd> grads;
    acq.batch_grad(Q, first, val, grads);
    for (const auto& g : grads)
        for (int d = 0; d < sh.D; ++d)
            gr.push_back(g(d));
    print_val("val", val);
    print_val("grad", gr);
    auto obj = limbo::opt::make_batch_objective(acq, first);
    print_val("obj", obj.batch(Q));
    if (sh.M > 0) {
        const limbo::opt::eval_t e = acq(Q[0], first, true);
        std::vector<double> one(1, std::get<0>(e));
        const Eigen::VectorXd g = std::get<1>(e).get();
        for (int d = 0; d < sh.D; ++d)
            one.push_back(g(d));
        print_val("single", one);
    }
    if (sh.n > 0) {
        std::mt19937_64 g((unsigned)Params::opt_batchgradsearch::seed()); // opt::BatchGradSearch's own candidates, as it draws them
        std::uniform_real_distribution<double> u01(0.0, 1.0);
        std::vector<Eigen::VectorXd> pts((size_t)Params::opt_batchgradsearch::points() + 1, Eigen::VectorXd(sh.D));
        pts[0] = Eigen::VectorXd::Constant(sh.D, 0.5);
        for (size_t i = 1; i < pts.size(); ++i)
            for (int d = 0; d < sh.D; ++d)
                pts[i](d) = u01(g);
        print_val("search_starts", acq.batch(pts, first));
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
    if (kind == 0 && mean == 2)
        return run<Params, kernel::SquaredExpARD<Params>, mean::Constant<Params>>(f, sh);
    if (kind == 1 && mean == 0)
        return run<Params, kernel::MaternFiveHalves<Params>, mean::Data<Params>>(f, sh);
    if (kind == 1 && mean == 2)
        return run<Params, kernel::MaternFiveHalves<Params>, mean::Constant<Params>>(f, sh);
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
    if (std::fscanf(f, "%d %d %d %d %d %d %d %d %d %lf %lf %lf", &kind, &mean, &sh.D, &sh.n, &sh.K, &sh.M, &noise_id, &sh.observation, &sh.nh,
            &sh.r[0], &sh.r[1], &sh.r[2])
        != 12)
        return 2;
    return noise_id == 1 ? dispatch<Params01>(f, kind, mean, sh) : dispatch<Params001>(f, kind, mean, sh);
}
