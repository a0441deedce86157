// sparse_grad.hip — kernels of the sparse pseudo-input GP's analytic gradient (include/gpe_sparse_grad.h; spgp.hpp:500-580).
//
// A chunk arrives in the transposed layout (points contiguous): Kt[n + j ldq] = K~_jn, and from the model's own V (the chunk as
// gpe_sp_compute solves it), scaled by 1 / sqrt(ep), three products on the matrix cores (gemm.hip): ILVt = Vt Lm^-T, B1t = ILVt Lt^-1,
// IQt = Vt L^-1.  Here:
//   k_sp_gcol    thread = point: mu, q, s -> bigsum, epc, (y~ - mu) / sig and the partial sums of the three scalars (:515-517, :554-562)
//   k_sp_grow    workgroup = (16 pseudo-inputs) x (slice of n): G in registers, its row sums against [1, x^, x^2] (:526-544)
//   k_sp_gfinish workgroup = pseudo-input: the sums against dnnQ, Q regenerated from Xb, the rescalings (:524-552)
//   k_sp_gscal   one workgroup: dfb, dfc, dfsig from the per-workgroup partials, in a fixed order (:546-562)
// Every sum runs in a fixed order (per-workgroup partials, folded in ascending index): no floating-point atomics.
// k_sp_grow reads the chunk's three buffers once per group of 8 dimensions: 24 M mc bytes against (2 + P + 17) M mc fused
// multiply-adds at D <= 8 — about one flop per byte, bound by memory, not by arithmetic.
#include <algorithm>

#include "dev.h"

namespace {
constexpr int RJ = 4;  // pseudo-inputs per wave of k_sp_grow
constexpr int RC = 8;  // dimensions per column group (2 RC + 1 sums per pseudo-input in registers)
constexpr int RSL_MAX = 64;
constexpr int RKMIN = 256; // no slice shorter

static __device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v += __shfl_down(v, o);
    return v; // lane 0
}
static __device__ __forceinline__ double block_sum4(double v, double* sh)
{
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0)
        sh[wv] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3]; // fixed order
}
} // namespace

int64_t sparse_grad_default_chunk(int64_t M)
{
    // the chunk's four M x chunk buffers (K~, B1, IQ, Lm^-1 V~) under 2^26 doubles = 512 MiB
    const int64_t c = (((int64_t)1 << 26) / (4 * std::max<int64_t>(M, 1))) / 64 * 64;
    return std::max<int64_t>(256, std::min<int64_t>(c, 65536));
}

int sparse_grad_row_slices(int64_t M, int64_t len, int cus)
{
    const int64_t jb = (M + 4 * RJ - 1) / (4 * RJ);
    int64_t s = (4 * (int64_t)cus + jb - 1) / jb;
    s = std::min<int64_t>(s, std::max<int64_t>(1, len / RKMIN));
    return (int)std::max<int64_t>(1, std::min<int64_t>(s, RSL_MAX));
}

// b1[j + p ldo] = sum_{k >= j} Lti[k + j ld] bet[k + p ldb]  (b1 = Lt^-T bet, Lti = Lt^-1 lower): workgroup = (j, p)
__global__ __launch_bounds__(256) void k_sp_gb1(const double* __restrict__ Lti, int64_t ld, int64_t M, const double* __restrict__ bet,
                                                int64_t ldb, double* __restrict__ b1, int64_t ldo)
{
    __shared__ double sh[4];
    const int64_t j = blockIdx.x;
    const int p = blockIdx.y;
    const double* col = Lti + j * ld;
    const double* bp = bet + (int64_t)p * ldb;
    double s = 0.0;
    for (int64_t k = j + threadIdx.x; k < M; k += 256)
        s = fma(col[k], bp[k], s);
    s = block_sum4(s, sh);
    if (threadIdx.x == 0)
        b1[j + (int64_t)p * ldo] = s;
}

__global__ void k_sp_grs(const double* __restrict__ ep, int64_t nc, double* __restrict__ rs)
{
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n < nc)
        rs[n] = 1.0 / sqrt(ep[n]);
}

// thread = point n of the chunk (one wave per workgroup, as k_sp_ep); reads along n are coalesced, the sums over j ascend.
// From ILVt = (Lm^-1 V~)^T — the reference's invLmV (:483) — and IQt: mu_np = bet_p . ILV_n (:509), q_n = |ILV_n|^2, s_n = |IQ_n|^2.
// big[n] = bigsum_n, R[n + p ldq] = (y~_np - mu_np) / sig, part[3 blk + {0, 1, 2}] = this workgroup's share of S_sig, S_epc, S_mu.
__global__ __launch_bounds__(64) void k_sp_gcol(const double* __restrict__ ILVt, const double* __restrict__ IQt, int64_t ldq, int64_t nc, int64_t M,
                                                const double* __restrict__ bet, int64_t ldbet, int P, const double* __restrict__ y, int64_t ldy,
                                                const double* __restrict__ ep, const double* __restrict__ rs, double c, double sig, double dl,
                                                double* __restrict__ big, double* __restrict__ R, double* __restrict__ part)
{
    const int64_t n0 = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const double f = n0 < nc ? 1.0 : 0.0;
    const int64_t n = n0 < nc ? n0 : nc - 1; // (a thread beyond the chunk reads the last point; its sums are cancelled by f)
    const double e = ep[n], r = rs[n];
    double q = 0.0, s = 0.0, acc = 0.0, smu = 0.0;
    for (int p0 = 0; p0 < P; p0 += 4) {
        const int pi[4] = {p0, min(p0 + 1, P - 1), min(p0 + 2, P - 1), min(p0 + 3, P - 1)};
        double mu[4] = {0.0, 0.0, 0.0, 0.0};
        const double* lp = ILVt + n;
        const double* ip = IQt + n;
        for (int64_t j = 0; j < M; ++j) {
            const double lv = lp[j * ldq];
            if (p0 == 0) { // (uniform)
                const double iq = ip[j * ldq];
                q = fma(lv, lv, q);
                s = fma(iq, iq, s);
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
                mu[a] = fma(bet[j + (int64_t)pi[a] * ldbet], lv, mu[a]);
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            if (p0 + a >= P)
                break;
            const double yy = y[n + (int64_t)pi[a] * ldy] * r;
            acc += yy * mu[a] / sig - (yy * yy + mu[a] * mu[a]) / (2.0 * sig); // spgp.hpp:515-517
            smu += mu[a] * (yy - mu[a]);
            if (n0 < nc)
                R[n + (int64_t)pi[a] * ldq] = (yy - mu[a]) / sig;
        }
    }
    const double bigsum = acc + (double)P * (0.5 - 0.5 * q);
    const double sumVsq = (c - (e - 1.0) * sig) / e; // sum_i V[i, n]^2 / ep_n from ep's definition (:399)
    const double epc = (c / e - sumVsq - dl * s) / sig; // :554-556
    if (n0 < nc)
        big[n] = bigsum;
    const double v0 = wave_sum(f * bigsum / e), v1 = wave_sum(f * epc * bigsum), v2 = wave_sum(f * smu);
    if (threadIdx.x == 0) {
        double* o = part + 3 * (int64_t)blockIdx.x;
        o[0] = v0;
        o[1] = v1;
        o[2] = v2;
    }
}

// Vst[n + i ldq] = rs[n] Z[n sn + i si]: the chunk's V in either layout of the model (sparse.hpp) -> V / sqrt(ep), transposed layout
__global__ __launch_bounds__(256) void k_sp_gvt(const double* __restrict__ Z, int64_t sn, int64_t si, int64_t nc, int64_t M,
                                                const double* __restrict__ rs, double* __restrict__ Vst, int64_t ldq)
{
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (n < nc && i < M)
        Vst[n + i * ldq] = rs[n] * Z[n * sn + i * si];
}

// T[j + i ld] = A[i + j ld], order M
__global__ __launch_bounds__(256) void k_sp_gtrans(const double* __restrict__ A, double* __restrict__ T, int64_t ld, int64_t M)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j < M && i < M)
        T[j + i * ld] = A[i + j * ld];
}

// Row sums of G against [1, x^, x^2].  Workgroup = (16 pseudo-inputs: 4 per wave) x (slice blockIdx.y of the chunk's points, cut
// at multiples of 64); lanes along n, so every read is coalesced.  G_jn is formed in registers, the features of the point come
// from the chunk's SoA coordinates; after the slice the 64 lanes are added by shuffles and lane 0 stores the slice's partial sums
// Part[((slice ncol + col) ldp) + j], col 0: g0, 1 + d: R1, 1 + D + d: R2.  Dimensions go in groups of RC (the three buffers are
// streamed once per group); a group's dimensions beyond D, a wave's pseudo-inputs beyond M and a slice's points beyond the chunk
// read a clamped address — no conditional loads — and are cancelled (the 0/1 factor f) or simply not stored.
__global__ __launch_bounds__(256) void k_sp_grow(const double* __restrict__ Kt, const double* __restrict__ B1t, const double* __restrict__ IQt,
                                                 int64_t ldq, int64_t nc, int64_t M, const double* __restrict__ b1, int64_t ldb1, int P,
                                                 const double* __restrict__ big, const double* __restrict__ R,
                                                 const double* __restrict__ Qt, KParams kp, double sig, int S, double* __restrict__ Part,
                                                 int64_t ldp)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int D = kp.Din;
    const int64_t j0 = ((int64_t)blockIdx.x * 4 + wv) * RJ;
    if (j0 >= M)
        return; // (whole wave; no barrier in this kernel)
    int64_t jj[RJ];
#pragma unroll
    for (int a = 0; a < RJ; ++a)
        jj[a] = min(j0 + a, M - 1);
    // the slice: units of 64 points, the first `rem` slices one unit longer (as the Gram's plan)
    const int64_t units = (nc + 63) / 64, base = units / S, rem = units % S, sl = blockIdx.y;
    const int64_t u0 = sl * base + min(sl, rem), u1 = u0 + base + (sl < rem ? 1 : 0);
    const int64_t k0 = u0 * 64, k1 = u1 * 64; // (k1 may exceed nc: clamped below)
    const double two_sig = 2.0 / sig, dP = (double)P;
    const int ncol = 2 * D + 1;
    double* out = Part + (int64_t)sl * ncol * ldp;
    for (int d0 = 0; d0 < D; d0 += RC) {
        double acc[RJ][2 * RC + 1];
#pragma unroll
        for (int a = 0; a < RJ; ++a)
#pragma unroll
            for (int cc = 0; cc < 2 * RC + 1; ++cc)
                acc[a][cc] = 0.0;
        int dd[RC];
        double ie[RC];
#pragma unroll
        for (int cc = 0; cc < RC; ++cc) {
            dd[cc] = min(d0 + cc, D - 1);
            ie[cc] = kp.inv_ell[dd[cc]];
        }
        for (int64_t nn = k0 + lane; nn < k1; nn += 64) {
            const double f = nn < nc ? 1.0 : 0.0;
            const int64_t n = nn < nc ? nn : nc - 1;
            const double bg = two_sig * big[n];
            double t[RJ], G[RJ];
#pragma unroll
            for (int a = 0; a < RJ; ++a)
                t[a] = 0.0;
            for (int p = 0; p < P; ++p) {
                const double rr = R[n + (int64_t)p * ldq];
#pragma unroll
                for (int a = 0; a < RJ; ++a)
                    t[a] = fma(b1[jj[a] + (int64_t)p * ldb1], rr, t[a]);
            }
#pragma unroll
            for (int a = 0; a < RJ; ++a) {
                const int64_t o = n + jj[a] * ldq;
                G[a] = f * Kt[o] * (dP * B1t[o] - bg * IQt[o] - t[a]);
                acc[a][0] += G[a];
            }
#pragma unroll
            for (int cc = 0; cc < RC; ++cc) {
                const double x = Qt[n + (int64_t)dd[cc] * ldq] * ie[cc], x2 = x * x;
#pragma unroll
                for (int a = 0; a < RJ; ++a) {
                    acc[a][1 + 2 * cc] = fma(G[a], x, acc[a][1 + 2 * cc]);
                    acc[a][2 + 2 * cc] = fma(G[a], x2, acc[a][2 + 2 * cc]);
                }
            }
        }
#pragma unroll
        for (int a = 0; a < RJ; ++a) {
            const bool live = j0 + a < M;
            const double g0 = wave_sum(acc[a][0]);
            if (lane == 0 && live && d0 == 0)
                out[j0 + a] = g0;
#pragma unroll
            for (int cc = 0; cc < RC; ++cc) {
                const double r1 = wave_sum(acc[a][1 + 2 * cc]), r2 = wave_sum(acc[a][2 + 2 * cc]);
                if (lane == 0 && live && d0 + cc < D) {
                    out[(int64_t)(1 + d0 + cc) * ldp + j0 + a] = r1;
                    out[(int64_t)(1 + D + d0 + cc) * ldp + j0 + a] = r2;
                }
            }
        }
    }
}

// Racc[j + col ldp] (=, first) or (+=) the S slices' partial sums in ascending slice
__global__ void k_sp_grow_fold(const double* __restrict__ Part, int64_t ldp, int ncol, int S, int first, int64_t M, double* __restrict__ Racc)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int col = blockIdx.y;
    if (j >= M)
        return;
    double s = Part[(int64_t)col * ldp + j];
    for (int q = 1; q < S; ++q)
        s += Part[((int64_t)q * ncol + col) * ldp + j];
    double* d = Racc + (int64_t)col * ldp + j;
    *d = first ? s : *d + s;
}

// Workgroup = pseudo-input j.  Q_jl is regenerated from the pseudo-inputs as k_build forms it (no jitter: dnnQ's diagonal is
// zero, and dfc wants Q - jitter I); W_jl = (-(b1 b1^T) + P (invQ - sig invA) - (2 / sig) TT)_jl Q_jl, and per dimension
// sum_l W_jl (x^b_jd - x^b_ld) (:524, :530-533 with the sums over n replaced by R1 - x^b g0).  Then the rescalings of :546-552:
// dxb[j D + d] is final; tb[j + d ldm] is pseudo-input j's share of dfb_d before its last factor sqrt(b_d) / 2.
// cs[j + {0, 1, 2, 3} ldm] = sum_l invA_jl (Q - jitter I)_jl, sum_l (b1 b1^T)_jl (Q - jitter I)_jl, invQ_jj, invA_jj (for dfc).
__global__ __launch_bounds__(256) void k_sp_gfinish(const double* __restrict__ Xt, int64_t ldx, KParams kp, int64_t M, int P,
                                                    const double* __restrict__ b1, int64_t ldb1, const double* __restrict__ IQm,
                                                    const double* __restrict__ IAm, const double* __restrict__ TT, int64_t ldm,
                                                    const double* __restrict__ Racc, double sig, double* __restrict__ dxb,
                                                    double* __restrict__ tb, double* __restrict__ cs)
{
    __shared__ double sh[4];
    const int D = kp.Din;
    const int64_t j = blockIdx.x;
    const double two_sig = 2.0 / sig, dP = (double)P;
    for (int d0 = 0; d0 < D; d0 += RC) {
        int dd[RC];
        double ie[RC], xj[RC], acc[RC];
#pragma unroll
        for (int cc = 0; cc < RC; ++cc) {
            dd[cc] = min(d0 + cc, D - 1);
            ie[cc] = kp.inv_ell[dd[cc]];
            xj[cc] = Xt[j + (int64_t)dd[cc] * ldx];
            acc[cc] = 0.0;
        }
        double sA = 0.0, sB = 0.0;
        for (int64_t l = threadIdx.x; l < M; l += 256) {
            double z = 0.0;
            for (int d = 0; d < D; ++d) {
                const double u = (Xt[j + (int64_t)d * ldx] - Xt[l + (int64_t)d * ldx]) * kp.inv_ell[d];
                z = fma(u, u, z);
            }
            const double Q = kp.sf2 * exp(-0.5 * z);
            double bb = 0.0;
            for (int p = 0; p < P; ++p)
                bb = fma(b1[j + (int64_t)p * ldb1], b1[l + (int64_t)p * ldb1], bb);
            const int64_t o = l + j * ldm; // (symmetric matrices: column j read along l)
            const double ia = IAm[o];
            const double w = (dP * (IQm[o] - sig * ia) - bb - two_sig * TT[o]) * Q;
            sA = fma(ia, Q, sA);
            sB = fma(bb, Q, sB);
#pragma unroll
            for (int cc = 0; cc < RC; ++cc)
                acc[cc] = fma(w, (xj[cc] - Xt[l + (int64_t)dd[cc] * ldx]) * ie[cc], acc[cc]);
        }
        if (d0 == 0) {
            sA = block_sum4(sA, sh);
            sB = block_sum4(sB, sh);
            if (threadIdx.x == 0) {
                cs[j] = sA;
                cs[j + ldm] = sB;
                cs[j + 2 * ldm] = IQm[j + j * ldm];
                cs[j + 3 * ldm] = IAm[j + j * ldm];
            }
        }
#pragma unroll
        for (int cc = 0; cc < RC; ++cc) {
            const double a = block_sum4(acc[cc], sh);
            if (threadIdx.x == 0 && d0 + cc < D) {
                const int d = d0 + cc;
                const double sqb = ie[cc], xb = xj[cc] * sqb;
                const double g0 = Racc[j], r1 = Racc[j + (int64_t)(1 + d) * ldm], r2 = Racc[j + (int64_t)(1 + D + d) * ldm];
                const double v = (a + r1 - xb * g0) * sqb;                  // :546
                dxb[j * D + d] = v;
                tb[j + (int64_t)d * ldm] = -(r2 - xb * r1) / sqb + v * xb / (sqb * sqb); // :548, :550
            }
        }
    }
}

static __device__ double strided_sum(const double* __restrict__ v, int64_t n, int64_t stride, double* sh)
{
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256)
        s += v[i * stride];
    return block_sum4(s, sh);
}

// one workgroup: dhp = { dfb_0 .. dfb_{D-1}, dfc, dfsig } (:552, :557-562)
__global__ __launch_bounds__(256) void k_sp_gscal(const double* __restrict__ part, int64_t nblk, const double* __restrict__ cs,
                                                  const double* __restrict__ tb, int64_t ldm, int64_t M, KParams kp, int P, double sig,
                                                  double dl, double* __restrict__ dhp)
{
    __shared__ double sh[4];
    const int D = kp.Din;
    const double s_sig = strided_sum(part, nblk, 3, sh), s_epc = strided_sum(part + 1, nblk, 3, sh), s_mu = strided_sum(part + 2, nblk, 3, sh);
    const double sA = strided_sum(cs, M, 1, sh), sB = strided_sum(cs + ldm, M, 1, sh);
    const double trQ = strided_sum(cs + 2 * ldm, M, 1, sh), trA = strided_sum(cs + 3 * ldm, M, 1, sh);
    for (int d = 0; d < D; ++d) {
        const double t = strided_sum(tb + (int64_t)d * ldm, M, 1, sh);
        if (threadIdx.x == 0)
            dhp[d] = t * kp.inv_ell[d] * 0.5;
    }
    if (threadIdx.x == 0) {
        // sum(invA o Q) = sA + jitter tr(invA)
        dhp[D] = (double)P * ((double)M + dl * (trQ - sig * trA) - sig * (sA + dl * trA)) * 0.5 - s_mu / sig + 0.5 * sB + s_epc;
        dhp[D + 1] = s_sig;
    }
}

void launch_sp_gb1(hipStream_t s, const double* Lti, int64_t ld, int64_t M, const double* bet, int64_t ldb, int P, double* b1, int64_t ldo)
{
    GPE_LAUNCH(k_sp_gb1, dim3((unsigned)M, (unsigned)P), dim3(256), 0, s, Lti, ld, M, bet, ldb, b1, ldo);
}
void launch_sp_grs(hipStream_t s, const double* ep, int64_t nc, double* rs)
{
    GPE_LAUNCH(k_sp_grs, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, s, ep, nc, rs);
}
void launch_sp_gcol(hipStream_t s, const double* ILVt, const double* IQt, int64_t ldq, int64_t nc, int64_t M, const double* bet, int64_t ldbet, int P,
                    const double* y, int64_t ldy, const double* ep, const double* rs, double c, double sig, double dl, double* big, double* R,
                    double* part)
{
    GPE_LAUNCH(k_sp_gcol, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, s, ILVt, IQt, ldq, nc, M, bet, ldbet, P, y, ldy, ep, rs, c, sig, dl, big, R,
               part);
}
void launch_sp_gvt(hipStream_t s, const double* Z, int64_t sn, int64_t si, int64_t nc, int64_t M, const double* rs, double* Vst, int64_t ldq)
{
    GPE_LAUNCH(k_sp_gvt, dim3((unsigned)((nc + 255) / 256), (unsigned)M), dim3(256), 0, s, Z, sn, si, nc, M, rs, Vst, ldq);
}
void launch_sp_gtrans(hipStream_t s, const double* A, double* T, int64_t ld, int64_t M)
{
    GPE_LAUNCH(k_sp_gtrans, dim3((unsigned)((M + 255) / 256), (unsigned)M), dim3(256), 0, s, A, T, ld, M);
}
void launch_sp_grow(hipStream_t s, const double* Kt, const double* B1t, const double* IQt, int64_t ldq, int64_t nc, int64_t M, const double* b1,
                    int64_t ldb1, int P, const double* big, const double* R, const double* Qt, const KParams& kp, double sig, int S, double* Part,
                    int64_t ldp, int first, double* Racc)
{
    const int ncol = 2 * kp.Din + 1;
    GPE_LAUNCH(k_sp_grow, dim3((unsigned)((M + 4 * RJ - 1) / (4 * RJ)), (unsigned)S), dim3(256), 0, s, Kt, B1t, IQt, ldq, nc, M, b1, ldb1, P, big, R,
               Qt, kp, sig, S, Part, ldp);
    GPE_LAUNCH(k_sp_grow_fold, dim3((unsigned)((M + 255) / 256), (unsigned)ncol), dim3(256), 0, s, Part, ldp, ncol, S, first, M, Racc);
}
void launch_sp_gfinish(hipStream_t s, const double* Xt, int64_t ldx, const KParams& kp, int64_t M, int P, const double* b1, int64_t ldb1,
                       const double* IQm, const double* IAm, const double* TT, int64_t ldm, const double* Racc, double sig, double dl,
                       const double* part, int64_t nblk, double* dxb, double* tb, double* cs, double* dhp)
{
    GPE_LAUNCH(k_sp_gfinish, dim3((unsigned)M), dim3(256), 0, s, Xt, ldx, kp, M, P, b1, ldb1, IQm, IAm, TT, ldm, Racc, sig, dxb, tb, cs);
    GPE_LAUNCH(k_sp_gscal, dim3(1), dim3(256), 0, s, part, nblk, cs, tb, ldm, M, kp, P, sig, dl, dhp);
}
