// ehvi.hip — the exact two-objective expected hypervolume improvement (include/gpe_ehvi.h): the strip kernel.
//
//   ehvi[m] = sum_{i = 0 .. n} (psi_1(l_i) - psi_1(l_{i+1})) psi_2(h_i),   psi_k(t) = s_k f((mu_k - t) / s_k),  f(z) = phi(z) + z Phi(z)
//
// l_0 = r1, l_i = y1(i), l_{n+1} = +inf (psi_1 = 0); h_i = y2(i+1), h_n = r2: strip i is the band l_i <= f1 < l_{i+1} above which
// the front reaches h_i.  psi falls with t, l rises, h falls: every term is positive (the reference's cell walk subtracts two
// products per cell and returns 0 where the value is 1e-60).  The partials in (mu2, s2) put Phi_2 / phi_2 in psi_2's place; those in
// (mu1, s1) are the same sum by parts, sum_i {Phi_1, phi_1}(l_i) (psi_2(h_i) - psi_2(h_{i-1})), psi_2(h_{-1}) = 0 — positive terms
// again, where the term-by-term derivative phi_1(l_i) - phi_1(l_{i+1}) changes sign.
//
// One wave per candidate, EHVI_W candidates per workgroup; the front sits in LDS as (y1, y2) pairs, shared by the waves.  Index
// i = 0 .. n + 1 goes to lane i mod 64 in rounds; the lane evaluates (psi, Phi, phi) of objective 1 at l_i and of objective 2 at
// h_i — two exp + erfc pairs — and takes index i - 1's values from the lane below (lane 0: from lane 63 of the round before).  With
// them it adds strip i - 1's term to the sums in (value, mu2, s2) and index i's to those in (mu1, s1).  Five accumulators per lane,
// ascending i; then one fixed xor tree over the 64 lanes and lane 0 stores.  The rounds are (n + 2 + 63) / 64 whatever the inputs;
// no workgroup waits for another; no atomics.  Nothing here is chosen from M.
#include <cfloat>

#include "belief.h"
#include "ehvi_forms.h" // ehvi_ev, ehvi_mul, ehvi_drop

namespace {
constexpr int EHVI_W = 4;            // waves = candidates per workgroup
constexpr int EHVI_T = 64 * EHVI_W;  // threads per workgroup
} // namespace

__global__ __launch_bounds__(EHVI_T) void k_ehvi2(EhviArgs q)
{
    extern __shared__ double2 ehvi_front[];
    const int n = q.n;
    for (int i = threadIdx.x; i < n; i += EHVI_T)
        ehvi_front[i] = make_double2(q.front[2 * i], q.front[2 * i + 1]);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * EHVI_W + (threadIdx.x >> 6);
    if (m >= q.M) // (wave-uniform; no barrier follows)
        return;

    const double mu1 = belief_mean(q.b, m, 0), mu2 = belief_mean(q.b, m, 1);
    const double sig = belief_shared_sigma(q.b, m); // (one model, two outputs)
    const double s1 = belief_sd(q.b, m, 0, sig), s2 = belief_sd(q.b, m, 1, sig);
    const double r1 = q.r1, r2 = q.r2, inf = __longlong_as_double(0x7ff0000000000000LL);

    double av = 0.0, am1 = 0.0, as1 = 0.0, am2 = 0.0, as2 = 0.0;
    double cA = 0.0, cPsi = 0.0, cPhi = 0.0, cphi = 0.0; // index i - 1 of lane 0: lane 63 of the round before
    const int rounds = (n + 2 + 63) / 64;
    for (int r = 0; r < rounds; ++r) {
        const int i = r * 64 + lane;
        Ev e1{0.0, 0.0, 0.0}, e2{0.0, 0.0, 0.0};
        double l = inf, lp = r1, h = r2, hp = r2; // l_i, l_{i-1}, h_i, h_{i-1}
        if (i <= n) {
            if (i >= 1) {
                const double2 p = ehvi_front[i - 1];
                l = p.x;
                hp = p.y;
            }
            else
                l = r1;
            if (i >= 2)
                lp = ehvi_front[i - 2].x;
            if (i < n)
                h = ehvi_front[i].y;
            e1 = ehvi_ev(mu1, s1, l);
            e2 = ehvi_ev(mu2, s2, h);
        }
        else if (i == n + 1 && n >= 1)
            lp = ehvi_front[n - 1].x;
        // index i - 1's values (every lane takes part in the shuffles)
        double pA = __shfl_up(e1.psi, 1), pPsi = __shfl_up(e2.psi, 1), pPhi = __shfl_up(e2.Phi, 1), pphi = __shfl_up(e2.phi, 1);
        if (lane == 0) {
            pA = cA;
            pPsi = cPsi;
            pPhi = cPhi;
            pphi = cphi;
        }
        cA = __shfl(e1.psi, 63);
        cPsi = __shfl(e2.psi, 63);
        cPhi = __shfl(e2.Phi, 63);
        cphi = __shfl(e2.phi, 63);
        if (i >= 1 && i <= n + 1) { // strip i - 1: l_{i-1} <= f1 < l_i at height h_{i-1}
            const double w = ehvi_drop(pA, e1.psi, l - lp);
            av += ehvi_mul(w, pPsi);
            am2 += ehvi_mul(w, pPhi);
            as2 += ehvi_mul(w, pphi);
        }
        if (i <= n) { // by parts: index i
            const double v = i == 0 ? e2.psi : ehvi_drop(e2.psi, pPsi, hp - h);
            am1 += ehvi_mul(e1.Phi, v);
            as1 += ehvi_mul(e1.phi, v);
        }
    }
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) {
        av += __shfl_xor(av, w);
        am1 += __shfl_xor(am1, w);
        as1 += __shfl_xor(as1, w);
        am2 += __shfl_xor(am2, w);
        as2 += __shfl_xor(as2, w);
    }
    if (lane != 0)
        return;
    q.ehvi[m] = av;
    if (q.partials) {
        q.partials[m] = am1;
        q.partials[m + q.ldp] = as1;
        q.partials[m + 2 * q.ldp] = am2;
        q.partials[m + 3 * q.ldp] = as2;
    }
    if (q.b.mu_out) {
        q.b.mu_out[m] = mu1;
        q.b.mu_out[m + q.b.ldm] = mu2;
    }
}

void launch_ehvi2(hipStream_t s, const EhviArgs& q)
{
    if (q.M <= 0 || q.n < 0)
        return;
    const size_t lds = sizeof(double2) * (size_t)(q.n > 0 ? q.n : 1);
    GPE_LAUNCH(k_ehvi2, dim3((unsigned)((q.M + EHVI_W - 1) / EHVI_W)), dim3(EHVI_T), lds, s, q);
}
