// ehvi3.hip — the exact three-objective expected hypervolume improvement (include/gpe_ehvi3.h): the box kernel.
//
//   ehvi[m] = sum_boxes (psi_a(l_a) - psi_a(u_a)) (psi_b(l_b) - psi_b(u_b)) psi_c(h),   psi_k(t) = s_k f((mu_k - t) / s_k)
//
// over the table of height axis c = 3 (ehvi3.hpp builds the tables on the host); the partials in (mu_c, s_c) put Phi_c / phi_c in
// psi_c's place and are taken from the table whose height axis is c, so that nothing but values of a falling psi is ever
// subtracted: every factor and every term of every sum is positive (the reference's schemes subtract whole products).
//
// One wave per candidate, EHVI3_W candidates per workgroup.  A table passes through LDS in pieces of EHVI3_PIECE boxes, one array
// per column, shared by the waves; box b of a table goes to lane b mod 64, in ceil(boxes / 64) rounds.  The lane evaluates psi of
// the two plane axes at the box's four thresholds and (psi, Phi, phi) of the height axis at h — five exp + erfc pairs — and adds the
// box's term to its three sums, ascending b; after a table one fixed xor tree over the 64 lanes, and lane 0 stores.  The rounds and
// the pieces are counted by the boxes alone, never by M or by a belief; a NaN belief takes the same steps as a finite one.  No
// workgroup waits for another; no atomics.
#include <cfloat>

#include "belief.h"
#include "ehvi_forms.h" // ehvi_ev, ehvi_mul, ehvi_drop

namespace {
constexpr int EHVI3_W = 4;             // waves = candidates per workgroup
constexpr int EHVI3_T = 64 * EHVI3_W;  // threads per workgroup
constexpr int EHVI3_PIECE = 512;       // boxes of a table in LDS at once: 20 KiB, eight rounds
} // namespace

// psi at a box's upper end: +inf (an unbounded strip) is psi = 0 whatever the belief — a NaN belief shows in psi at the lower end
static __device__ __forceinline__ double ehvi3_psi_up(double mu, double s, double u)
{
    const double psi = ehvi_ev(mu, s, u).psi;
    return u > DBL_MAX ? 0.0 : psi;
}

__global__ __launch_bounds__(EHVI3_T) void k_ehvi3(Ehvi3Args q)
{
    __shared__ double box[5 * EHVI3_PIECE];
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * EHVI3_W + (threadIdx.x >> 6);
    const bool live = m < q.M; // (wave-uniform; a wave past M still fills LDS and meets the barriers)

    double mu0 = 0.0, mu1 = 0.0, mu2 = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (live) {
        mu0 = belief_mean(q.b, m, 0);
        mu1 = belief_mean(q.b, m, 1);
        mu2 = belief_mean(q.b, m, 2);
        const double sig = belief_shared_sigma(q.b, m); // (one model, three outputs)
        s0 = belief_sd(q.b, m, 0, sig);
        s1 = belief_sd(q.b, m, 1, sig);
        s2 = belief_sd(q.b, m, 2, sig);
    }

    const double* tab = q.tables;
    for (int t = 0; t < q.ntab; ++t) {
        const int c = t == 0 ? 2 : t - 1; // the height axis; a < b: the other two
        const double mua = c == 0 ? mu1 : mu0, sa = c == 0 ? s1 : s0;
        const double mub = c == 2 ? mu1 : mu2, sb = c == 2 ? s1 : s2;
        const double muc = c == 0 ? mu0 : (c == 1 ? mu1 : mu2), sc = c == 0 ? s0 : (c == 1 ? s1 : s2);
        const int nb = q.nb[t];
        double av = 0.0, am = 0.0, as = 0.0;
        for (int p0 = 0; p0 < nb; p0 += EHVI3_PIECE) {
            const int cnt = min(EHVI3_PIECE, nb - p0);
            __syncthreads(); // the piece before is consumed
            for (int i = threadIdx.x; i < 5 * cnt; i += EHVI3_T)
                box[(i % 5) * EHVI3_PIECE + i / 5] = tab[5 * (int64_t)p0 + i];
            __syncthreads();
            if (live)
                for (int r = lane; r < cnt; r += 64) {
                    const double la = box[r], ua = box[EHVI3_PIECE + r], lb = box[2 * EHVI3_PIECE + r], ub = box[3 * EHVI3_PIECE + r];
                    const double wa = ehvi_drop(ehvi_ev(mua, sa, la).psi, ehvi3_psi_up(mua, sa, ua), ua - la);
                    const double wb = ehvi_drop(ehvi_ev(mub, sb, lb).psi, ehvi3_psi_up(mub, sb, ub), ub - lb);
                    const Ev e = ehvi_ev(muc, sc, box[4 * EHVI3_PIECE + r]);
                    const double w = ehvi_mul(wa, wb);
                    av += ehvi_mul(w, e.psi);
                    am += ehvi_mul(w, e.Phi);
                    as += ehvi_mul(w, e.phi);
                }
        }
        tab += 5 * (int64_t)nb;
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) {
            av += __shfl_xor(av, w);
            am += __shfl_xor(am, w);
            as += __shfl_xor(as, w);
        }
        if (live && lane == 0) {
            if (t == 0)
                q.ehvi[m] = av;
            if (q.partials) {
                q.partials[m + 2 * c * q.ldp] = am;
                q.partials[m + (2 * c + 1) * q.ldp] = as;
            }
        }
    }
    if (live && lane == 0 && q.b.mu_out) {
        q.b.mu_out[m] = mu0;
        q.b.mu_out[m + q.b.ldm] = mu1;
        q.b.mu_out[m + 2 * q.b.ldm] = mu2;
    }
}

void launch_ehvi3(hipStream_t s, const Ehvi3Args& q)
{
    if (q.M <= 0 || q.ntab < 1)
        return;
    GPE_LAUNCH(k_ehvi3, dim3((unsigned)((q.M + EHVI3_W - 1) / EHVI3_W)), dim3(EHVI3_T), 0, s, q);
}
