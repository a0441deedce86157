// nei.hip — noisy expected improvement in the log domain (include/gpe_nei.h): the kernels.
//
//   lognei[m] = log((1 / S) sum_s exp(term_s)),   term_s = log sd + log h((cmean[s, m] - fplus[s] - xi) / sd),   h = phi + z Phi
//
// Every draw s of the function at the baseline points brings its own incumbent fplus[s] and its own mean cmean[s, m] at the
// candidate; the standard deviation sd is the same for all of them.  Conditioning on a draw leaves little variance near the
// baseline, so z runs to the hundreds below zero where h as written is 0: log h comes from logh.h (cei.hip's forms: Mills' ratio
// as a positive continued fraction of fixed depth below z = -3, the direct forms above).
//
// k_lognei: one WAVE per candidate, NEI_W waves per workgroup, fplus in LDS for the workgroup.  Lane l owns the samples l, l + 64,
// ..: at most NEI_PER = 16 terms, kept in registers (the loop over them is not unrolled — sixteen copies of the fraction would
// not fit the instruction cache — and a term reaches its register through a chain of selects on the wave-uniform loop index).  The
// candidate's cmean column is contiguous: a wave's loads are.  The maximum is taken first, then the sum of exp(term - max): per
// lane over its samples ascending, across the lanes in __shfl_xor trees — an order fixed by S alone.  The region branches of log h
// diverge within a wave; each side is then run once.  No atomics, nothing chosen from M: a candidate's numbers are bitwise the same
// in any batch.
//
// k_nei_colmax: fplus[s] = max_i F[i, s], one wave per draw.  k_nei_cond: per candidate, one wave: |u|^2 of its column of U = L_b^-1 c
// (lanes over the baseline points ascending, a __shfl_xor tree), cvar = var - |u|^2, the mean mu as used, and the S entries of its
// cmean column set to mu, for the matrix-core product Z^T U to be added to.
#include "belief.h" // the clamp
#include "logh.h"

namespace {
constexpr int NEI_W = 4;          // waves (candidates) per workgroup
constexpr int NEI_T = 64 * NEI_W; // threads per workgroup
constexpr int NEI_PER = 16;       // samples per lane: GPE_NEI_MAX_SAMPLES / 64
} // namespace

__global__ __launch_bounds__(NEI_T) void k_lognei(NeiArgs q)
{
    extern __shared__ __attribute__((aligned(16))) double nei_lds[]; // S: fplus
    const int S = q.S;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < S; k += NEI_T)
        nei_lds[k] = q.fplus[k];
    __syncthreads();
    const int64_t m = (int64_t)blockIdx.x * NEI_W + wave;
    if (m >= q.M) // (wave-uniform; no barrier follows)
        return;
    const double inf = __longlong_as_double(0x7ff0000000000000LL), nan = __longlong_as_double(0x7ff8000000000000LL);

    double sd;
    if (q.cvar)
        sd = belief_sigma(q.cvar[m], 0.0);
    else
        sd = q.csd[m];
    const double lsd = log(sd); // (sd = 0: not used)
    const double* cm = q.cmean + m * q.ldm;

    double t[NEI_PER];
#pragma unroll
    for (int j = 0; j < NEI_PER; ++j)
        t[j] = -inf;
    double top = -inf;
    bool bad = sd != sd;
    const int per = (S + 63) >> 6;
#pragma unroll 1
    for (int i = 0; i < per; ++i) {
        const int k = lane + 64 * i;
        double term = -inf;
        if (k < S) {
            const double d = cm[k] - nei_lds[k] - q.xi;
            if (sd == 0.0) // no uncertainty left: the improvement itself, or none
                term = d > 0.0 ? log(d) : (d != d ? d : -inf);
            else {
                double lh, rP, rp;
                cei_log_h(d / sd, lh, rP, rp);
                term = lsd + lh;
            }
        }
        bad |= term != term;
        top = fmax(top, term);
#pragma unroll
        for (int j = 0; j < NEI_PER; ++j)
            t[j] = j == i ? term : t[j];
        if (q.terms && k < S)
            q.terms[k + m * q.ldt] = term;
    }
#pragma unroll
    for (int w = 32; w > 0; w >>= 1)
        top = fmax(top, __shfl_xor(top, w));
    double val;
    if (__any(bad))
        val = nan;
    else if (top == inf || top == -inf)
        val = top; // a mean of +inf: +inf; every term -inf: -inf
    else {
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < NEI_PER; ++j)
            if (lane + 64 * j < S)
                sum += exp(t[j] - top);
#pragma unroll
        for (int w = 32; w > 0; w >>= 1)
            sum += __shfl_xor(sum, w);
        val = top + log(sum) - log((double)S);
    }
    if (q.terms && val != val) // NaN for that candidate alone — and for all of it
        for (int k = lane; k < S; k += 64)
            q.terms[k + m * q.ldt] = nan;
    if (lane == 0)
        q.lognei[m] = val;
}

void launch_lognei(hipStream_t s, const NeiArgs& q)
{
    if (q.M <= 0 || q.S < 1 || q.S > 64 * NEI_PER)
        return;
    GPE_LAUNCH(k_lognei, dim3((unsigned)((q.M + NEI_W - 1) / NEI_W)), dim3(NEI_T), sizeof(double) * (size_t)q.S, s, q);
}

__global__ __launch_bounds__(64) void k_nei_colmax(const double* __restrict__ F, int64_t B, int S, double* __restrict__ fplus)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= S)
        return;
    double top = -__longlong_as_double(0x7ff0000000000000LL);
    for (int64_t i = lane; i < B; i += 64)
        top = fmax(top, F[i + (int64_t)s * B]);
#pragma unroll
    for (int w = 32; w > 0; w >>= 1)
        top = fmax(top, __shfl_xor(top, w));
    if (lane == 0)
        fplus[s] = top;
}

void launch_nei_colmax(hipStream_t s, const double* F, int64_t B, int S, double* fplus)
{
    if (B <= 0 || S <= 0)
        return;
    GPE_LAUNCH(k_nei_colmax, dim3((unsigned)S), dim3(64), 0, s, F, B, S, fplus);
}

__global__ __launch_bounds__(NEI_T) void k_nei_cond(const double* __restrict__ U, int64_t ldu, int64_t B, const double* __restrict__ kta,
                                                     const double* __restrict__ add, const double* __restrict__ var, int64_t M, int S,
                                                     double* __restrict__ mu_out, double* __restrict__ cvar, double* __restrict__ cmean,
                                                     int64_t ldm)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t m = (int64_t)blockIdx.x * NEI_W + wave;
    if (m >= M)
        return;
    const double* u = U + m * ldu;
    double ss = 0.0;
    for (int64_t i = lane; i < B; i += 64)
        ss += u[i] * u[i];
#pragma unroll
    for (int w = 32; w > 0; w >>= 1)
        ss += __shfl_xor(ss, w);
    const double mu = add ? kta[m] + add[m] : kta[m];
    if (lane == 0) {
        mu_out[m] = mu;
        cvar[m] = var[m] - ss;
    }
    for (int k = lane; k < S; k += 64)
        cmean[k + m * ldm] = mu;
}

void launch_nei_cond(hipStream_t s, const double* U, int64_t ldu, int64_t B, const double* kta, const double* add, const double* var, int64_t M,
                     int S, double* mu_out, double* cvar, double* cmean, int64_t ldm)
{
    if (M <= 0)
        return;
    GPE_LAUNCH(k_nei_cond, dim3((unsigned)((M + NEI_W - 1) / NEI_W)), dim3(NEI_T), 0, s, U, ldu, B, kta, add, var, M, S, mu_out, cvar, cmean, ldm);
}
