// kg.hip — the knowledge gradient over a finite alternative set (include/gpe_kg.h): the envelope kernel.
//
//   kg[m] = h(a, b) = E_Z[max_i (a_i + b_i Z)] - max_i a_i,   b = column m of B (given scaled, or scaled here from cov and var)
//
// h is Frazier's sum over the breakpoints of the upper envelope of the lines a_i + b_i z: sum (b_next - b_cur) f(-|z|),
// f(z) = phi(z) + z Phi(z) — every term positive, nothing cancels (E[max] - max a does).  The envelope is a SUCCESSOR CHAIN: for
// line i, over all j with b_j > b_i, z_ij = (a_i - a_j) / (b_j - b_i); hi_i = min_j z_ij and succ_i its arg-min (the lowest j on
// exact ties).  The chain starts at the smallest slope (ties: the largest a, then the lowest index) and follows succ: each step goes
// to a strictly larger slope, so it ends, and no per-line "alive" test decides anything.  The walk is bounded by the line count
// regardless (NaN / inf inputs).
//
// One workgroup per candidate.  (a_j, b_j) sit in LDS as pairs: the sweep over j reads them with one 16-byte broadcast read per
// wave (every lane the same address: no bank conflicts), a thread owns lines tid, tid + 256, .. in blocks of KG_R registers.  The
// O(A^2) pair steps are one fp64 division each; hi / succ go to LDS and one lane walks them.  Fixed order throughout, no atomics.
#include <cfloat>

#include "logh.h" // the normal constants

namespace {
constexpr int KG_T = 256; // threads per workgroup
constexpr int KG_R = 4;   // lines a thread sweeps at once
} // namespace

// f(-|z|) = phi - |z| Phi(-|z|) >= 0.  Loses about z^2 ulps to cancellation at large |z|; the clamp only matters where phi is
// denormal; |z| = inf gives 0 (not inf * 0)
static __device__ __forceinline__ double kg_f(double z)
{
    const double t = -fabs(z);
    if (!(t >= -DBL_MAX)) // -inf or NaN
        return t != t ? t : 0.0;
    const double phi = exp(-0.5 * t * t) * LOGH_INV_SQRT2PI;
    const double Phi = 0.5 * erfc(-t * LOGH_INV_SQRT2);
    return fmax(phi + t * Phi, 0.0);
}

// a: A means; B: column m at B + m ldb, A slopes — scaled already (var == null) or the unscaled covariance column, scaled here by
// 1 / sqrt(var[m] + obs_noise).  with_self (var != null only): line A = (mu_c[m], var[m] / sqrt(var[m] + obs_noise)).
// LDS: (nl) pairs, nl doubles hi, nl ints succ, nl <= GPE_KG_MAX_ALTERNATIVES + 1.
__global__ __launch_bounds__(KG_T) void k_kg_envelope(const double* __restrict__ a, int A, const double* __restrict__ B, int64_t ldb,
                                                      const double* __restrict__ var, double obs_noise, int with_self,
                                                      const double* __restrict__ mu_c, double* __restrict__ kg, int* __restrict__ nseg)
{
    extern __shared__ double2 kg_lds[];
    __shared__ double rb[KG_T], ra[KG_T];
    __shared__ int ri[KG_T];
    const int64_t m = blockIdx.x;
    const int tid = threadIdx.x;
    const int nl = A + (var && with_self ? 1 : 0);
    double2* ab = kg_lds;
    double* hi = (double*)(ab + nl);
    int* succ = (int*)(hi + nl);

    double rs = 1.0, d = 1.0;
    if (var) {
        d = var[m] + obs_noise;
        if (!(d > DBL_EPSILON) || !(d <= DBL_MAX)) { // nothing can be learnt there (uniform: every thread reads the same word)
            if (tid == 0) {
                kg[m] = 0.0;
                if (nseg)
                    nseg[m] = 0;
            }
            return;
        }
        rs = sqrt(d);
    }
    const double* bcol = B + m * ldb;
    for (int i = tid; i < A; i += KG_T)
        ab[i] = make_double2(a[i], var ? bcol[i] / rs : bcol[i]);
    if (nl > A && tid == 0)
        ab[A] = make_double2(mu_c[m], var[m] / rs);
    __syncthreads();

    // the sweep: hi_i, succ_i of the thread's lines, and the thread's candidate for the start of the chain
    double sb = 0.0, sa = 0.0;
    int si = -1;
    for (int i0 = tid; i0 < nl; i0 += KG_T * KG_R) {
        double ai[KG_R], bi[KG_R], h[KG_R];
        int sc[KG_R];
#pragma unroll
        for (int r = 0; r < KG_R; ++r) {
            const int i = i0 + r * KG_T;
            const double2 v = ab[i < nl ? i : i0];
            ai[r] = v.x;
            bi[r] = v.y;
            h[r] = __longlong_as_double(0x7ff0000000000000LL); // +inf
            sc[r] = -1;
        }
        for (int j = 0; j < nl; ++j) {
            const double2 v = ab[j];
#pragma unroll
            for (int r = 0; r < KG_R; ++r) {
                if (v.y > bi[r]) {
                    const double z = (ai[r] - v.x) / (v.y - bi[r]);
                    if (z < h[r] || sc[r] < 0) { // (ascending j and a strict <: the lowest j of equal z; the first steeper line always counts)
                        h[r] = z;
                        sc[r] = j;
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < KG_R; ++r) {
            const int i = i0 + r * KG_T;
            if (i < nl) {
                hi[i] = h[r];
                succ[i] = sc[r];
                if (si < 0 || bi[r] < sb || (bi[r] == sb && ai[r] > sa)) { // (ascending i: the lowest index of equal lines)
                    sb = bi[r];
                    sa = ai[r];
                    si = i;
                }
            }
        }
    }
    rb[tid] = sb;
    ra[tid] = sa;
    ri[tid] = si;
    __syncthreads();
    for (int w = KG_T / 2; w > 0; w >>= 1) {
        if (tid < w) {
            const int oi = ri[tid + w], mi = ri[tid];
            const double ob = rb[tid + w], oa = ra[tid + w];
            if (oi >= 0 && (mi < 0 || ob < rb[tid] || (ob == rb[tid] && (oa > ra[tid] || (oa == ra[tid] && oi < mi))))) {
                rb[tid] = ob;
                ra[tid] = oa;
                ri[tid] = oi;
            }
        }
        __syncthreads();
    }
    if (tid != 0)
        return;
    // the walk: at most nl - 1 steps can be real (slopes strictly ascend); the bound holds for any input
    int i = ri[0], steps = 0;
    double h = 0.0;
    while (i >= 0 && steps < nl) {
        const int j = succ[i];
        if (j < 0)
            break;
        h += (ab[j].y - ab[i].y) * kg_f(hi[i]);
        i = j;
        ++steps;
    }
    kg[m] = h;
    if (nseg)
        nseg[m] = steps;
}

static size_t kg_envelope_lds(int nl) { return (size_t)nl * (sizeof(double2) + sizeof(double) + sizeof(int)); }

void launch_kg_envelope(hipStream_t s, const double* a, int A, const double* B, int64_t ldb, int64_t M, const double* var, double obs_noise,
                        int with_self, const double* mu_c, double* kg, int* nseg)
{
    if (M <= 0 || A <= 0)
        return;
    const int nl = A + (var && with_self ? 1 : 0);
    GPE_LAUNCH(k_kg_envelope, dim3((unsigned)M), dim3(KG_T), kg_envelope_lds(nl), s, a, A, B, ldb, var, obs_noise, with_self, mu_c, kg, nseg);
}
