// Driver for the knowledge gradient through the drop-in model::GP (knowledge_gradient, acqui/kg.hpp).  Where the model lives is
// decided as everywhere by Params::gpu::min_n_for_gpu() / LIMBO_AMD_MIN_N_FOR_GPU: with a large value nothing touches the device
// and the driver runs on a box WITHOUT a GPU (tests/test_kg_host.py), with the default the larger models run on it
// (tests/test_gpu_kg.py).
//   test_kg_dropin <input file> : kind mean P D n A M agg with_self noise_id nh, then nh log hyper-parameters (0: the functor's
//                                 defaults), n rows of X (D) and Y (P), A alternatives (D), M candidates (D)
//   agg 0: the FirstElem aggregator, 1: the second output;  noise_id 0: kernel noise 0.01, 1: 0.1
// prints: host_resident; kg (limbo_amd::kg_batch); best (limbo_amd::kg_best); plain (knowledge_gradient with no means passed:
// k^T alpha of output 0, the kernel's noise); A + M <= 128: mu ((A + M) x P) and cov ((A + M)^2) of query_joint over the
// alternatives followed by the candidates, column-major — the beliefs the envelope was given.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <limbo/acqui/kg.hpp>
#include <limbo/kernel/matern_five_halves.hpp>
#include <limbo/kernel/squared_exp_ard.hpp>
#include <limbo/mean/constant.hpp>
#include <limbo/mean/data.hpp>
#include <limbo/model/gp.hpp>

struct ParamsBase {
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

struct SecondElem {
    typedef double result_type;
    double operator()(const Eigen::VectorXd& x) const { return x(1); }
};

static void print_val(const char* name, const std::vector<double>& v)
{
    std::printf("%s", name);
    for (double x : v)
        std::printf(" %.17g", x);
    std::printf("\n");
}

struct Shape {
    int P, D, n, A, M, agg, with_self, nh;
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
    std::vector<Eigen::VectorXd> H, XY, X, Y, Qa, Qc;
    if (!rows(sh.nh > 0 ? 1 : 0, sh.nh, H) || !rows(sh.n, sh.D + sh.P, XY) || !rows(sh.A, sh.D, Qa) || !rows(sh.M, sh.D, Qc))
        return 2;
    for (const auto& r : XY) {
        Eigen::VectorXd x(sh.D), y(sh.P);
        for (int d = 0; d < sh.D; ++d)
            x(d) = r(d);
        for (int p = 0; p < sh.P; ++p)
            y(p) = r(sh.D + p);
        X.push_back(x);
        Y.push_back(y);
    }
    limbo::model::GP<Params, Kernel, Mean> gp(sh.D, sh.P);
    if (sh.nh > 0)
        gp.kernel_function().set_h_params(H[0]);
    if (sh.n > 0)
        gp.compute(X, Y);
    std::printf("host_resident %d\n", (int)gp.host_resident());
    std::vector<double> kg;
    int64_t best;
    if (sh.agg == 1) {
        kg = limbo_amd::kg_batch<Params>(gp, Qa, Qc, SecondElem(), sh.with_self != 0);
        best = limbo_amd::kg_best<Params>(gp, Qa, Qc, SecondElem(), sh.with_self != 0);
    }
    else {
        kg = limbo_amd::kg_batch<Params>(gp, Qa, Qc, limbo_amd::FirstElem(), sh.with_self != 0);
        best = limbo_amd::kg_best<Params>(gp, Qa, Qc, limbo_amd::FirstElem(), sh.with_self != 0);
    }
    print_val("kg", kg);
    std::printf("best %lld\n", (long long)best);
    std::vector<double> plain;
    gp.knowledge_gradient(Qa, Qc, sh.with_self != 0, plain);
    print_val("plain", plain);
    if (sh.A + sh.M <= 128) {
        std::vector<Eigen::VectorXd> pts(Qa);
        pts.insert(pts.end(), Qc.begin(), Qc.end());
        Eigen::MatrixXd mu, cov;
        gp.query_joint(pts, mu, cov);
        print_val("mu", std::vector<double>(mu.data(), mu.data() + mu.size()));
        print_val("cov", std::vector<double>(cov.data(), cov.data() + cov.size()));
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
    if (std::fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d", &kind, &mean, &sh.P, &sh.D, &sh.n, &sh.A, &sh.M, &sh.agg, &sh.with_self, &noise_id, &sh.nh)
        != 11)
        return 2;
    return noise_id == 1 ? dispatch<Params01>(f, kind, mean, sh) : dispatch<Params001>(f, kind, mean, sh);
}
