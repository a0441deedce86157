// mes.hip — max-value entropy search in the log domain (include/gpe_mes.h): the kernel.
//
//   terms[m, j] = log((1 / K) sum_k t(g_jk)),  g_jk = (ystar[k, j] - mu_j) / s_j,  t(g) = g phi(g) / (2 Phi(g)) - log Phi(g)
//   logmes[m]   = log sum_j exp(terms[m, j])
//
// t as written is 0 / 0 below g = -38.5 and exactly 0, hence flat, above g = +38.6.  Here log t and r = t' / t come from three forms,
// with x = |g|, Mills' ratio R(x) = Phi(-x) / phi(x), 1 / T = x + c2, c2 = 2 / (x + 3 / (x + ...)) (logh.h's fraction; the inner tail
// IS c2, so 1 - x T = c2 T is never formed by subtraction) and lambda = phi / Phi:
//   g < -LOGH_XC   lambda = x + T     t = log sqrt(2 pi) + log(x + T) - x T / 2     (>= 2 minus <= 1 / 2)      t' = -(lambda / 2) c2 T
//   g > +LOGH_XC   Q = phi R          log t = -g^2 / 2 - log sqrt(2 pi) + log B,  B = g / (2 (1 - Q)) + R (-log1p(-Q) / Q)   (all > 0)
//                                    t' / t = -[1 + g (g + phi / (1 - Q))] / (2 (1 - Q) B)                      (no phi left: -> -g)
//   otherwise     t = g lambda / 2 - log Phi,   t' = -(lambda / 2) (1 + g (g + lambda))
// The fraction is evaluated bottom-up from quotient LOGH_DEPTH whatever x is: at x = LOGH_XC that leaves 2.4e-17 of T,
// less at every larger x, and at x = 1e100 every step is x + k / x = x.
//
// One WAVE per candidate, MES_W waves per workgroup.  For each output j in turn the workgroup stages ystar's column j in LDS, shared
// by its waves; a wave's lanes take the samples k = lane, lane + 64, ...: the work is J K chains of dependent fp64 divisions, and one
// thread per candidate would run K = 1024 of them back to back.  Pass one leaves log t and r of every sample in the wave's own LDS
// rows and finds the maximum; pass two sums exp(log t - max) and its products with r and g r.  Maximum and sums cross the lanes in
// __shfl_xor trees, per lane they run over k ascending: an order fixed by K alone.  Lane j keeps output j's term and partials; the
// log-sum-exp over j is a tree over lanes 0 .. 7.  The region branches diverge within a wave; each side is then run once.  No atomics,
// nothing chosen from M: a candidate's numbers are bitwise the same in any batch.
#include "belief.h"
#include "logh.h" // the constants and logh_c2

namespace {
constexpr int MES_W = 2;           // waves (candidates) per workgroup
constexpr int MES_T = 64 * MES_W;  // threads per workgroup
} // namespace

// log t(g) and r = t'(g) / t(g) <= 0.  g = -inf: (+inf, 0); g = +inf: (-inf, 0); NaN: NaN.
static __device__ __forceinline__ void mes_log_t(double g, double& lt, double& r)
{
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    const double x = fabs(g);
    if (x == inf) {
        lt = g < 0.0 ? inf : -inf;
        r = 0.0;
        return;
    }
    if (x > LOGH_XC) {
        const double c2 = logh_c2(x), T = 1.0 / (x + c2);
        if (g < 0.0) {
            const double lam = x + T;
            const double t = LOGH_LOG_SQRT2PI + log(lam) - 0.5 * x * T;
            lt = log(t);
            r = -(0.5 * lam) * c2 * T / t;
        }
        else {
            const double phi = exp(-0.5 * x * x) * LOGH_INV_SQRT2PI;
            const double R = 1.0 / (x + T);
            const double Q = phi * R, P = 1.0 - Q;
            const double quot = Q > 0.0 ? -log1p(-Q) / Q : 1.0;
            const double B = x / (2.0 * P) + R * quot;
            lt = -0.5 * x * x - LOGH_LOG_SQRT2PI + log(B);
            r = -(1.0 + x * (x + phi / P)) / (2.0 * P * B);
        }
        return;
    }
    const double phi = exp(-0.5 * x * x) * LOGH_INV_SQRT2PI;
    const double Q = 0.5 * erfc(x * LOGH_INV_SQRT2);
    const double Phi = g < 0.0 ? Q : 1.0 - Q;
    const double lP = g < 0.0 ? log(Q) : log1p(-Q);
    const double lam = phi / Phi;
    const double t = 0.5 * g * lam - lP;
    lt = log(t);
    r = -(0.5 * lam) * (1.0 + g * (g + lam)) / t;
}

__global__ __launch_bounds__(MES_T) void k_mes(MesArgs q)
{
    extern __shared__ double mes_lds[];
    const int K = q.K, J = q.J;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* ys = mes_lds;                                  // K: ystar's column j
    double* wlt = mes_lds + K + (size_t)wave * 2 * K;      // K: the wave's log t
    double* wr = wlt + K;                                  // K: the wave's r
    const int64_t m = (int64_t)blockIdx.x * MES_W + wave;
    const bool live = m < q.M; // (wave-uniform; every wave takes part in the barriers)
    const double inf = __longlong_as_double(0x7ff0000000000000LL), nan = __longlong_as_double(0x7ff8000000000000LL);
    const double logK = log((double)K);

    const double sig = live ? belief_shared_sigma(q.b, m) : 0.0; // (one model, several outputs)
    double term = -inf, pm = 0.0, ps = 0.0; // lane j < J: output j's

    for (int j = 0; j < J; ++j) {
        __syncthreads(); // the column before is read out
        for (int k = threadIdx.x; k < K; k += MES_T)
            ys[k] = q.ystar[k + (size_t)j * K];
        __syncthreads();
        if (!live)
            continue;
        const double mu = belief_mean(q.b, m, j);
        if (q.b.mu_out && lane == 0)
            q.b.mu_out[m + (int64_t)j * q.b.ldm] = mu;
        const double s = belief_sd(q.b, m, j, sig);
        double tj, mj = 0.0, sj = 0.0;
        if (mu != mu || s != s)
            tj = mj = sj = nan;
        else if (s == 0.0) // nothing to learn about this output
            tj = -inf;
        else {
            double top = -inf;
            bool bad = false;
            for (int k = lane; k < K; k += 64) {
                double lt, r;
                mes_log_t((ys[k] - mu) / s, lt, r);
                wlt[k] = lt;
                wr[k] = r;
                bad |= lt != lt;
                top = fmax(top, lt);
            }
#pragma unroll
            for (int w = 32; w > 0; w >>= 1)
                top = fmax(top, __shfl_xor(top, w));
            if (__any(bad))
                tj = mj = sj = nan; // (an infinite mu beside an infinite s)
            else if (top == inf || top == -inf)
                tj = top; // mu = +inf: +inf; mu = -inf: -inf; the partials are 0
            else {
                double S = 0.0, A = 0.0, G = 0.0;
                for (int k = lane; k < K; k += 64) { // (the lane reads what it wrote)
                    const double e = exp(wlt[k] - top), r = wr[k];
                    S += e;
                    A += e * r;
                    G += e * (((ys[k] - mu) / s) * r);
                }
#pragma unroll
                for (int w = 32; w > 0; w >>= 1) {
                    S += __shfl_xor(S, w);
                    A += __shfl_xor(A, w);
                    G += __shfl_xor(G, w);
                }
                tj = top + log(S) - logK;
                mj = -(A / S) / s;
                sj = -(G / S) / s;
            }
        }
        if (lane == j) {
            term = tj;
            pm = mj;
            ps = sj;
        }
    }
    if (!live)
        return;

    // log sum_j exp(term_j): lanes 0 .. 7 (lanes >= J hold -inf and add exp(-inf) = 0)
    double top = term;
    bool bad = term != term;
#pragma unroll
    for (int w = 4; w > 0; w >>= 1)
        top = fmax(top, __shfl_xor(top, w));
    bad = __any(bad && lane < 8);
    double val, wj;
    if (bad)
        val = wj = nan;
    else if (top == inf || top == -inf) {
        val = top;
        wj = 0.0;
    }
    else {
        const double e = exp(term - top);
        double S = e;
#pragma unroll
        for (int w = 4; w > 0; w >>= 1)
            S += __shfl_xor(S, w);
        val = top + log(S);
        wj = e / S;
    }
    if (lane == 0 && q.logmes)
        q.logmes[m] = val;
    if (lane < J) {
        if (q.terms)
            q.terms[m + (int64_t)lane * q.ldt] = bad ? nan : term;
        if (q.partials) {
            q.partials[m + (int64_t)lane * q.ldp] = wj == 0.0 ? 0.0 : wj * pm;
            q.partials[m + (int64_t)(J + lane) * q.ldp] = wj == 0.0 ? 0.0 : wj * ps;
        }
    }
}

void launch_mes(hipStream_t s, const MesArgs& q)
{
    if (q.M <= 0 || q.J < 1 || q.J > 8 || q.K < 1 || q.K > 1024)
        return;
    const size_t lds = sizeof(double) * (size_t)q.K * (1 + 2 * MES_W);
    GPE_LAUNCH(k_mes, dim3((unsigned)((q.M + MES_W - 1) / MES_W)), dim3(MES_T), lds, s, q);
}
