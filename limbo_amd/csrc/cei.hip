// cei.hip — constrained expected improvement in the log domain (include/gpe_cei.h): the kernel.
//
//   logcei[m] = [with_ei] (log s0 + log h(z)) + sum_k log Phi(u_k),   h(z) = phi(z) + z Phi(z),  z = (mu0 - f_best - xi) / s0,
//                                                                     u_k = (mu_k - t_k) / s_k
//
// h is the difference of two nearly equal numbers for z < 0 and underflows to 0 below z = -38.6 (acqui::EI, kg.hip's kg_f and
// ehvi.hip's ehvi_ev form it as written and say so).  Here, for z < -LOGH_XC, with x = -z and Mills' ratio R(x) = Phi(-x) / phi(x),
//   h(z) = Phi(z) T(x),  T(x) = 1 / R(x) - x = 1 / (x + 2 / (x + 3 / (x + ...))),   1 / R(x) = x + T(x)
// every partial quotient positive, nothing subtracted:
//   log Phi(-x) = -x^2 / 2 - log sqrt(2 pi) - log(x + T)        lambda(-x) = phi / Phi = x + T
//   log h(-x)   = log Phi(-x) - log(1 / T)                      Phi / h = 1 / T,  phi / h = (x + T) / T
// The fraction is evaluated bottom-up from quotient LOGH_DEPTH whatever x is: at x = LOGH_XC that leaves 2.4e-17 of T, less
// at every larger x, and at x = 1e100 every step is x + k / x = x.  Above the crossover the direct forms: phi - |z| Q(|z|) cancels
// at most 1 / (1 - 3 R(3)) = 11.6 times there, and for z >= 0 it is added to z.
//
// One thread per candidate, 64 per workgroup (one wave: 16 384 candidates are 256 waves, one per compute unit — the thread's work
// is a chain of dependent fp64 divisions, so waves spread out finish sooner than waves packed).  The beliefs are column-major: a
// wave's loads are contiguous.  The loop over the constraints has the wave-uniform bound C; thresholds and columns come from the
// kernel's arguments.  The two region branches per belief diverge within a wave of mixed candidates; each side is then run once.
// No LDS, no atomics, nothing chosen from M: a candidate's numbers are bitwise the same in any batch.
#include "belief.h"
#include "logh.h" // the constants, logh_inv_T and cei_log_h

namespace {
constexpr int CEI_T = 64; // threads per workgroup
} // namespace

// log Phi(u) with lambda(u) = phi(u) / Phi(u).  u = -inf: (-inf, inf); u = +inf: (0, 0); NaN: NaN.
static __device__ __forceinline__ void cei_log_Phi(double u, double& lP, double& lam)
{
    if (u < -LOGH_XC) {
        const double x = -u, rinv = x + 1.0 / logh_inv_T(x);
        lP = -0.5 * x * x - LOGH_LOG_SQRT2PI - log(rinv);
        lam = rinv;
        return;
    }
    const double a = fabs(u);
    const double phi = exp(-0.5 * a * a) * LOGH_INV_SQRT2PI;
    const double Q = 0.5 * erfc(a * LOGH_INV_SQRT2);
    if (u < 0.0) {
        lP = log(Q);
        lam = phi / Q;
    }
    else {
        lP = log1p(-Q);
        lam = phi / (1.0 - Q);
    }
}

__global__ __launch_bounds__(CEI_T) void k_logcei(CeiArgs q)
{
    const int64_t m = (int64_t)blockIdx.x * CEI_T + threadIdx.x;
    if (m >= q.M)
        return;
    const double ninf = __longlong_as_double(0xfff0000000000000LL);
    const int C = q.C;
    const double sig = belief_shared_sigma(q.b, m); // (one model, several outputs)
    double total = 0.0;
    bool any_nan = false, any_ninf = false;

    if (q.with_ei || q.b.mu_out) {
        const double mu0 = belief_mean(q.b, m, 0);
        if (q.b.mu_out)
            q.b.mu_out[m] = mu0;
        double t0 = 0.0, pm = 0.0, ps = 0.0;
        if (q.with_ei) {
            const double s = belief_sd(q.b, m, 0, sig);
            const double d = mu0 - q.f_best - q.xi;
            if (s == 0.0) { // no uncertainty: the improvement itself, or none
                t0 = d > 0.0 ? log(d) : (d != d ? d : ninf);
                pm = d > 0.0 ? 1.0 / d : (d != d ? d : 0.0);
                ps = d != d ? d : 0.0;
            }
            else {
                double lh, rP, rp;
                cei_log_h(d / s, lh, rP, rp);
                t0 = log(s) + lh;
                pm = rP / s;
                ps = rp / s;
            }
            total = t0;
            any_nan = t0 != t0;
            any_ninf = t0 == ninf;
        }
        if (q.terms)
            q.terms[m] = t0;
        if (q.partials) {
            q.partials[m] = pm;
            q.partials[m + q.ldp] = ps;
        }
    }
    else {
        if (q.terms)
            q.terms[m] = 0.0;
        if (q.partials)
            q.partials[m] = q.partials[m + q.ldp] = 0.0;
    }

    for (int k = 0; k < C; ++k) {
        const double mu = belief_mean(q.b, m, 1 + k);
        if (q.b.mu_out)
            q.b.mu_out[m + (int64_t)(1 + k) * q.b.ldm] = mu;
        const double s = belief_sd(q.b, m, 1 + k, sig);
        const double d = mu - q.thr[k];
        double term, pm, ps;
        if (s == 0.0) { // no uncertainty: met or not
            term = d >= 0.0 ? 0.0 : (d != d ? d : ninf);
            pm = ps = d != d ? d : 0.0;
        }
        else {
            const double u = d / s;
            double lam;
            cei_log_Phi(u, term, lam);
            pm = lam / s;
            ps = lam == 0.0 ? 0.0 : -(u * lam) / s; // (inf 0 at u = +inf)
        }
        total += term;
        any_nan |= term != term;
        any_ninf |= term == ninf;
        if (q.terms)
            q.terms[m + (int64_t)(1 + k) * q.ldt] = term;
        if (q.partials) {
            q.partials[m + (int64_t)(2 + k) * q.ldp] = pm;
            q.partials[m + (int64_t)(2 + C + k) * q.ldp] = ps;
        }
    }
    if (total != total && !any_nan && any_ninf) // +inf (mu0 = +inf) beside -inf (a constraint surely missed): not feasible
        total = ninf;
    if (q.logcei)
        q.logcei[m] = total;
}

void launch_logcei(hipStream_t s, const CeiArgs& q)
{
    if (q.M <= 0 || q.C < 0 || q.C > 16)
        return;
    GPE_LAUNCH(k_logcei, dim3((unsigned)((q.M + CEI_T - 1) / CEI_T)), dim3(CEI_T), 0, s, q);
}
