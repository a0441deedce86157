// limbo/model/gp/host_small.hpp — the exact-GP linear algebra for SMALL models on the host (an addition; not in limbo).
//
// Below Params::gpu::min_n_for_gpu() samples a GP is cheaper to keep on the host than on the device: one add_sample() or one
// single-point query() is O(n^2) flops — 11-18 us on one core at n = 200 — while ANY per-call device path pays a kernel launch
// and a PCIe round trip first (measured: 24-28 us through the one-launch kernels of csrc/small.hip).  limbo's
// stock acquisition optimisers call query() thousands of times per iteration on models of 10..200 samples
// (src/limbo/bayes_opt/boptimizer.hpp:148-161, src/benchmarks/limbo/bench.cpp:66-84), and its own test asserts that an
// incremental update beats a full recompute at n = 100 (src/tests/test_gp.cpp:625-628).
//
// What is here is what model::GP needs in that regime and nothing else, written against raw column-major storage (so that
// it compiles with Eigen3 and with the minimal stand-in alike):
//   llt_lower        K = L L^T in place (right-looking, column by column: contiguous axpys)           gp.hpp:565
//   append_row       the new row of L for one more sample (forward substitution + sqrt)                 gp.hpp:591-597
//   solve_lower / solve_lower_t   L y = b, L^T x = y for P right-hand sides                             gp.hpp:608-610, :620
// Everything above the threshold, every batched query, K^-1, the gradients and the LOO objectives stay on the device.
#ifndef LIMBO_MODEL_GP_HOST_SMALL_HPP
#define LIMBO_MODEL_GP_HOST_SMALL_HPP
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include <limbo/tools/macros.hpp>

namespace limbo {
    namespace defaults {
        /// samples below which a model::GP keeps its factor on the host (0: always on the device).  256 = where one core's
        /// O(n^2) call meets the device's launch + PCIe floor, and the limit of the device's one-launch small path.
        struct gpu_host {
            BO_PARAM(int, min_n_for_gpu, 256);
        };
    } // namespace defaults
} // namespace limbo

namespace limbo_amd {
    /// Params::gpu::min_n_for_gpu() when the user's Params has it, defaults::gpu_host::min_n_for_gpu() otherwise;
    /// LIMBO_AMD_MIN_N_FOR_GPU in the environment overrides both (tests, benchmarks)
    template <typename Params, typename = void>
    struct param_min_n {
        static int get() { return limbo::defaults::gpu_host::min_n_for_gpu(); }
    };
    template <typename Params>
    struct param_min_n<Params, decltype((void)Params::gpu::min_n_for_gpu())> {
        static int get() { return Params::gpu::min_n_for_gpu(); }
    };
    template <typename Params>
    inline int min_n_for_gpu()
    {
        static const int env = [] {
            const char* e = std::getenv("LIMBO_AMD_MIN_N_FOR_GPU");
            return e ? std::atoi(e) : -1;
        }();
        return env >= 0 ? env : param_min_n<Params>::get();
    }

    /// query_batch() on a host-resident model goes to the device from this many (points x samples) on: below it the
    /// per-point host loop is cheaper than refreshing the device copy and a launch (LIMBO_AMD_HOST_BATCH_CROSSOVER)
    inline long host_batch_crossover()
    {
        static const long v = [] {
            const char* e = std::getenv("LIMBO_AMD_HOST_BATCH_CROSSOVER");
            return e ? std::atol(e) : 4096L;
        }();
        return v;
    }

    /// query_batch() of a device-resident model is dealt over ALL visible devices (one replica each, a host thread per
    /// device) from this many points on (LIMBO_AMD_MULTI_DEVICE_QUERY_MIN; 0: never) — the reference's parallel query
    /// (multi_gp.hpp:191-195, tools/parallel.hpp:138-201) with GPUs in place of cores
    inline long multi_device_query_min()
    {
        static const long v = [] {
            const char* e = std::getenv("LIMBO_AMD_MULTI_DEVICE_QUERY_MIN");
            return e ? std::atol(e) : 16384L;
        }();
        return v;
    }

    namespace host_small {
        /// A (n x n, column-major, leading dimension lda): lower triangle in, L out; the strict upper triangle is zeroed
        /// (gp.hpp:565: `Eigen::LLT<MatrixXd>(K).matrixL()` is dense with a zero upper part).  Returns 0, or the 1-based
        /// index of the first non-positive pivot (NaNs propagate from there on, as they do in the reference).
        inline int llt_lower(double* A, int64_t n, int64_t lda)
        {
            int bad = 0;
            for (int64_t j = 0; j < n; ++j) {
                double* cj = A + j * lda;
                const double d = cj[j];
                if (!(d > 0.0) && !bad)
                    bad = (int)(j + 1);
                const double l = std::sqrt(d), inv = 1.0 / l;
                cj[j] = l;
                for (int64_t i = j + 1; i < n; ++i)
                    cj[i] *= inv;
                for (int64_t k = j + 1; k < n; ++k) { // trailing columns: a_ik -= l_ij l_kj, i >= k
                    double* ck = A + k * lda;
                    const double lkj = cj[k];
                    for (int64_t i = k; i < n; ++i)
                        ck[i] -= cj[i] * lkj;
                }
                for (int64_t i = 0; i < j; ++i)
                    cj[i] = 0.0;
            }
            return bad;
        }
        /// L y = b in place for P right-hand sides (B: n x P, column-major, ldb)
        inline void solve_lower(const double* L, int64_t n, int64_t ldl, double* B, int64_t P, int64_t ldb)
        {
            for (int64_t p = 0; p < P; ++p) {
                double* b = B + p * ldb;
                for (int64_t j = 0; j < n; ++j) {
                    const double* cj = L + j * ldl;
                    const double y = b[j] / cj[j];
                    b[j] = y;
                    for (int64_t i = j + 1; i < n; ++i)
                        b[i] -= cj[i] * y;
                }
            }
        }
        /// L^T x = y in place
        inline void solve_lower_t(const double* L, int64_t n, int64_t ldl, double* B, int64_t P, int64_t ldb)
        {
            for (int64_t p = 0; p < P; ++p) {
                double* b = B + p * ldb;
                for (int64_t j = n - 1; j >= 0; --j) {
                    const double* cj = L + j * ldl;
                    double s = b[j];
                    for (int64_t i = j + 1; i < n; ++i)
                        s -= cj[i] * b[i];
                    b[j] = s / cj[j];
                }
            }
        }
        /// The row that one more sample appends to L (gp.hpp:591-597): kcol[0..n) = k(x_i, x_new), knn = k(x_new, x_new) +
        /// noise + 1e-8.  row[0..n) = L^-1 kcol, row[n] = sqrt(knn - |row|^2).  Returns 0, or n + 1 for a non-positive pivot.
        inline int append_row(const double* L, int64_t n, int64_t ldl, const double* kcol, double knn, double* row)
        {
            for (int64_t i = 0; i < n; ++i)
                row[i] = kcol[i];
            for (int64_t j = 0; j < n; ++j) {
                const double* cj = L + j * ldl;
                const double y = row[j] / cj[j];
                row[j] = y;
                for (int64_t i = j + 1; i < n; ++i)
                    row[i] -= cj[i] * y;
            }
            double s = 0.0;
            for (int64_t i = 0; i < n; ++i)
                s += row[i] * row[i];
            const double d = knn - s;
            row[n] = std::sqrt(d);
            return d > 0.0 ? 0 : (int)(n + 1);
        }
        /// Rows and columns R[0] < R[1] < ... < R[q-1] leave the factor L (order n, ldl): out (order n - q, ldo, strict upper
        /// triangle zeroed) = chol(K[S, S]), S the kept set in its order (include/gpe_remove.h).  The column sweep: a removed
        /// column's part below its diagonal becomes an update vector, a kept column takes one Givens rotation with every live
        /// vector, chosen from (L[c, c], u[c]) — a positive rank-1 update each, so no pivot can fail.  NaNs propagate.
        inline void remove_rows(const double* L, int64_t n, int64_t ldl, const int64_t* R, int64_t q, double* out, int64_t ldo)
        {
            std::vector<double> U((size_t)(n * q), 0.0), col((size_t)n);
            std::vector<int64_t> newrow((size_t)n);
            for (int64_t r = 0, k = 0; r < n; ++r) {
                if (k < q && R[k] == r) {
                    newrow[(size_t)r] = -1;
                    ++k;
                }
                else
                    newrow[(size_t)r] = r - k;
            }
            int64_t born = 0, cn = 0;
            for (int64_t c = 0; c < n; ++c) {
                const double* cj = L + c * ldl;
                if (newrow[(size_t)c] < 0) {
                    double* u = U.data() + born * n;
                    for (int64_t r = c + 1; r < n; ++r)
                        u[r] = cj[r];
                    ++born;
                    continue;
                }
                for (int64_t r = c; r < n; ++r)
                    col[(size_t)r] = cj[r];
                for (int64_t v = 0; v < born; ++v) {
                    double* u = U.data() + v * n;
                    const double d = col[(size_t)c], uc = u[c];
                    if (uc == 0.0)
                        continue;
                    const double h = std::hypot(d, uc), cs = d / h, sn = uc / h;
                    col[(size_t)c] = h;
                    u[c] = 0.0;
                    for (int64_t r = c + 1; r < n; ++r) {
                        const double x = col[(size_t)r], y = u[r];
                        col[(size_t)r] = cs * x + sn * y;
                        u[r] = -sn * x + cs * y;
                    }
                }
                double* oj = out + cn * ldo;
                for (int64_t i = 0; i < cn; ++i)
                    oj[i] = 0.0;
                for (int64_t r = c; r < n; ++r)
                    if (newrow[(size_t)r] >= 0)
                        oj[newrow[(size_t)r]] = col[(size_t)r];
                ++cn;
            }
        }
        /// The score of one candidate in greedy batch selection (include/gpe_batch_select.h): rule 0 UCB (param = beta), 1 EI
        /// (param = f+ + jitter; acqui/ei.hpp: _value), 2 the variance; var_add enters behind the clamp of gp.hpp:623
        inline double select_score(int rule, double mu, double var, double var_add, double param)
        {
            const double s2 = (var <= 2.220446049250313e-16 ? 0.0 : var) + var_add;
            if (rule == 2)
                return s2;
            const double sigma = std::sqrt(s2);
            if (rule == 0)
                return mu + param * sigma;
            if (sigma < 1e-10)
                return 0.0;
            const double X = mu - param, Z = X / sigma;
            const double phi = std::exp(-0.5 * Z * Z) / std::sqrt(2.0 * M_PI);
            const double Phi = 0.5 * std::erfc(-Z / std::sqrt(2));
            return X * Phi + sigma * phi;
        }
        /// The recursion of include/gpe_batch_select.h on a full posterior covariance Sig (M x M, column-major, lds; no jitter
        /// on its diagonal): q greedy picks, each followed by a rank-1 downdate of the variance by a hallucinated observation
        /// of noise obs_noise.  W: M x q scratch (ld M) that holds the columns afterwards; var: M, out (var_q, no clamp);
        /// idx, score: q.  Returns 0, or t + 1 for the first round t whose pivot is not positive (idx / score of rounds <= t
        /// are set).
        inline int select_greedy(const double* Sig, int64_t M, int64_t lds, const double* mu, int q, int rule, double param, double var_add,
            double obs_noise, bool distinct, int64_t* idx, double* score, double* var, double* W)
        {
            for (int64_t m = 0; m < M; ++m)
                var[m] = Sig[m + m * lds];
            for (int t = 0; t < q; ++t) {
                int64_t j = -1;
                double best = 0.0;
                for (int64_t m = 0; m < M; ++m) {
                    bool taken = false;
                    for (int s = 0; distinct && s < t && !taken; ++s)
                        taken = idx[s] == m;
                    if (taken)
                        continue;
                    const double v = select_score(rule, mu[m], var[m], var_add, param);
                    if (v == v && (j < 0 || v > best)) { // (ascending m: `>` keeps the lowest index of equal values)
                        best = v;
                        j = m;
                    }
                }
                idx[t] = j;
                score[t] = j < 0 ? std::nan("") : best;
                if (j < 0)
                    return t + 1;
                double* w = W + (int64_t)t * M;
                for (int64_t m = 0; m < M; ++m) {
                    double c = Sig[m + j * lds];
                    for (int s = 0; s < t; ++s)
                        c -= W[m + (int64_t)s * M] * W[j + (int64_t)s * M];
                    w[m] = c;
                }
                const double piv = w[j] + obs_noise;
                if (!(piv > 0.0) || !std::isfinite(piv))
                    return t + 1;
                const double r = std::sqrt(piv);
                for (int64_t m = 0; m < M; ++m) {
                    w[m] /= r;
                    var[m] -= w[m] * w[m];
                }
            }
            return 0;
        }
    } // namespace host_small
} // namespace limbo_amd
#endif
