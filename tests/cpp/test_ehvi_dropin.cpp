// Driver for the two-objective expected hypervolume improvement through the drop-in (model::GP::expected_hypervolume_improvement,
// acqui/ehvi.hpp).  Where the models live is decided as everywhere by Params::gpu::min_n_for_gpu() / LIMBO_AMD_MIN_N_FOR_GPU: with a
// large value nothing touches the device and the driver runs on a box WITHOUT a GPU (tests/test_ehvi_host.py), with the default the
// larger models run on it (tests/test_gpu_ehvi.py).
//   test_ehvi_dropin <input file> : kind mean D n K M noise_id observation nh r1 r2, then nh log hyper-parameters (0: the functor's
//                                   defaults), n rows of X (D) and Y (2), K objective points (2) the front is taken from, M candidates (D)
// prints: host_resident (the two-output model, and the two one-output models); front (row-major) and hv (pareto_front2, hypervolume2);
// one / best_one (ehvi2_batch, ehvi2_best on ONE model with two outputs) with mu (M x 2 column-major) and s2 (sigma^2 as query_batch
// reports it: the noise included) it worked from; two / best_two (the same on TWO one-output models) with mu1, s2_1, mu2, s2_2;
// val / grad (acqui::Ehvi2::batch_grad; grad row-major M x D), obj (Ehvi2 through opt::make_batch_objective) and single (operator()
// of candidate 0 with its gradient: value, then D numbers).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <limbo/acqui/ehvi.hpp>
#include <limbo/kernel/matern_five_halves.hpp>
#include <limbo/kernel/squared_exp_ard.hpp>
#include <limbo/mean/constant.hpp>
#include <limbo/mean/data.hpp>
#include <limbo/model/gp.hpp>
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
    double r1, r2;
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
    std::vector<Eigen::VectorXd> H, XY, X, Y, Y1, Y2, Fp, Q;
    if (!rows(sh.nh > 0 ? 1 : 0, sh.nh, H) || !rows(sh.n, sh.D + 2, XY) || !rows(sh.K, 2, Fp) || !rows(sh.M, sh.D, Q))
        return 2;
    for (const auto& r : XY) {
        Eigen::VectorXd x(sh.D), y(2), y1(1), y2(1);
        for (int d = 0; d < sh.D; ++d)
            x(d) = r(d);
        y(0) = y1(0) = r(sh.D);
        y(1) = y2(0) = r(sh.D + 1);
        X.push_back(x);
        Y.push_back(y);
        Y1.push_back(y1);
        Y2.push_back(y2);
    }
    using GP = limbo::model::GP<Params, Kernel, Mean>;
    GP gp(sh.D, 2), g1(sh.D, 1), g2(sh.D, 1);
    if (sh.nh > 0)
        for (GP* g : {&gp, &g1, &g2})
            g->kernel_function().set_h_params(H[0]);
    if (sh.n > 0) {
        gp.compute(X, Y);
        g1.compute(X, Y1);
        g2.compute(X, Y2);
    }
    std::printf("host_resident %d %d %d\n", (int)gp.host_resident(), (int)g1.host_resident(), (int)g2.host_resident());
    Eigen::VectorXd ref(2);
    ref << sh.r1, sh.r2;
    const std::vector<double> front = limbo_amd::pareto_front2(Fp, ref);
    print_val("front", front);
    std::printf("hv %.17g\n", limbo_amd::hypervolume2(front, ref));
    const bool obs = sh.observation != 0;

    print_val("one", limbo_amd::ehvi2_batch<Params>(gp, Q, front, ref, 0, 1, obs));
    std::printf("best_one %lld\n", (long long)limbo_amd::ehvi2_best<Params>(gp, Q, front, ref, 0, 1, obs));
    print_val("swapped", limbo_amd::ehvi2_batch<Params>(gp, Q, front, ref, 1, 0, obs)); // (objectives exchanged: only for its statuses and shape)
    std::printf("best_none %lld\n", (long long)limbo_amd::ehvi2_best<Params>(gp, std::vector<Eigen::VectorXd>(), front, ref));
    Eigen::MatrixXd mu;
    Eigen::VectorXd s2;
    gp.query_batch(Q, mu, s2);
    print_val("mu", flat(mu));
    print_val("s2", flat(s2));

    print_val("two", limbo_amd::ehvi2_batch<Params>(g1, g2, Q, front, ref, limbo_amd::FirstElem(), obs));
    std::printf("best_two %lld\n", (long long)limbo_amd::ehvi2_best<Params>(g1, g2, Q, front, ref, limbo_amd::FirstElem(), obs));
    g1.query_batch(Q, mu, s2);
    print_val("mu1", flat(mu));
    print_val("s2_1", flat(s2));
    g2.query_batch(Q, mu, s2);
    print_val("mu2", flat(mu));
    print_val("s2_2", flat(s2));

    limbo::acqui::Ehvi2<Params, GP> acq(g1, g2, front, ref, obs);
    std::vector<double> val, gr;
    std::vector<Eigen::VectorXd> grads;
    acq.batch_grad(Q, limbo_amd::FirstElem(), val, grads);
    for (const auto& g : grads)
        for (int d = 0; d < sh.D; ++d)
            gr.push_back(g(d));
    print_val("val", val);
    print_val("grad", gr);
    const limbo_amd::FirstElem first;
    print_val("obj", limbo::opt::make_batch_objective(acq, first).batch(Q));
    if (sh.M > 0) {
        const limbo::opt::eval_t e = acq(Q[0], first, true);
        std::vector<double> one(1, std::get<0>(e));
        const Eigen::VectorXd g = std::get<1>(e).get();
        for (int d = 0; d < sh.D; ++d)
            one.push_back(g(d));
        print_val("single", one);
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
    if (std::fscanf(f, "%d %d %d %d %d %d %d %d %d %lf %lf", &kind, &mean, &sh.D, &sh.n, &sh.K, &sh.M, &noise_id, &sh.observation, &sh.nh, &sh.r1,
            &sh.r2)
        != 11)
        return 2;
    return noise_id == 1 ? dispatch<Params01>(f, kind, mean, sh) : dispatch<Params001>(f, kind, mean, sh);
}
