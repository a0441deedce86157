// pathwise.hip — posterior draws as functions (include/gpe_pathwise.h): the two sums of a path and its gradient,
//   F[t, c]  = mean + sum_r amp cos(om_r . x_t + b_r) W[r, c]        + sum_i k(x_t, x_i) U[i, c]
//   dF[t, c] =      - sum_r amp sin(om_r . x_t + b_r) om_r W[r, c]   + sum_i g(z_ti) Mm (x_t - x_i) U[i, c]
// by ONE kernel in two modes: both are "a scalar basis function of the point and its gradient, times a coefficient matrix".  Host
// side: pathwise.hpp.
//
// Rows.  As everywhere in the engine a point is its D inputs and, for SE-ARD with Lambda, the k projections Lambda^T x (R = D + k
// rows, kp.D), and the kernels work on the rows scaled by s_r = 1 / ell_r (1 on the projection rows).  In these rows
//   om_r . x = sum_row Omega0[r, row] (s_row x_row)     (the scaling of the frequencies by the hyper-parameters, gpe_pathwise.h)
//   z        = sum_row (s_row (v_row - x_row))^2        (qgrad.hip)
// and both gradients are accumulated in the rows as they stand; the fold kernel applies s_d and Lambda once per point, as
// k_query_grad_fold does.  amp = sqrt(2 sf2 / R) is folded into the device copy of W when the set is made.
#include "dev.h"
#include "kfun_fast.h"

#define PW_LANES 64 // thread = point; one wave per workgroup
enum { PW_FEATURE = 0, PW_KERNEL = 1 };

// part[((seg ncol + c) NS + slot) ldp + m]: slot 0 the value, slot 1 + row the gradient in row `row` (NS = 1 + R; RT = 0: the value
// alone, NS = 1), summed over the basis functions of segment seg in ascending order.
//   grid: x = 64-point groups, y = segments of the basis functions (equal lengths), z = (row tile, column tile)
//   LDS : qs[R][64] the workgroup's points (scaled), each lane its own column
// Bt — Omega0 by rows (FEATURE) or the samples by rows, scaled by s_r when the set was made (KERNEL) —, the phases and the
// coefficients are the same for every lane: they are read straight from memory at wave-uniform addresses, which the compiler turns
// into scalar loads, and enter the FMAs as scalar operands.  (Staged in LDS they cost one broadcast read per FMA: the LDS port, not
// the FMA pipe, then bounds the loop.)
// One sincos / one exp per (point, basis function), reused across the CT columns and the RT rows of the tile; the phase / z is
// recomputed over all R rows in every row tile (as k_query_grad).  The value is accumulated in every row tile by the same
// instructions in the same order — F of a value-only launch is bitwise F of a gradient launch — and stored by row tile 0.
template <int MODE, int RT, int CT>
__global__ __launch_bounds__(PW_LANES) void k_paths_basis(const double* __restrict__ Qt, int64_t ldq, int64_t M,
                                                          const double* __restrict__ Bt, int64_t ldb, int64_t NB,
                                                          const double* __restrict__ phase, const double* __restrict__ Cf, int64_t ldc,
                                                          int ncol, KParams kp, double* __restrict__ part, int64_t ldp)
{
    extern __shared__ __attribute__((aligned(16))) double pw_lds[];
    constexpr int RTT = RT > 0 ? RT : 1;
    const int R = kp.D, lane = threadIdx.x;
    double* qs = pw_lds; // R x 64
    const int row_tiles = RT > 0 ? (R + RT - 1) / RT : 1, NS = RT > 0 ? 1 + R : 1;
    const int r0 = ((int)blockIdx.z % row_tiles) * RTT, c0 = ((int)blockIdx.z / row_tiles) * CT;
    const int64_t m = (int64_t)blockIdx.x * PW_LANES + lane, mc = m < M ? m : M - 1;
    const int64_t nseg = gridDim.y, seg = blockIdx.y;
    const int64_t len = (NB + nseg - 1) / nseg, i0 = seg * len, i1 = i0 + len < NB ? i0 + len : NB;

    for (int r = 0; r < R; ++r)
        qs[r * PW_LANES + lane] = Qt[mc + (int64_t)r * ldq] * kp.inv_ell[r];
    double qr[RTT], acc[CT], g[RTT][CT];
    const double* brow[RTT]; // the tile's rows of Bt (rows beyond R: the last one again, never stored)
    const double* ccol[CT];  // the tile's columns of Cf (columns beyond ncol: the last one again, never stored)
#pragma unroll
    for (int a = 0; a < RTT; ++a) {
        const int r = r0 + a < R ? r0 + a : R - 1;
        qr[a] = Qt[mc + (int64_t)r * ldq] * kp.inv_ell[r];
        brow[a] = Bt + (int64_t)r * ldb;
#pragma unroll
        for (int b = 0; b < CT; ++b)
            g[a][b] = 0.0;
    }
#pragma unroll
    for (int b = 0; b < CT; ++b) {
        acc[b] = 0.0;
        ccol[b] = Cf + (int64_t)(c0 + b < ncol ? c0 + b : ncol - 1) * ldc;
    }

    for (int64_t i = i0; i < i1; ++i) {
        double bv, gv; // the basis function and the scalar factor of its gradient
        if (MODE == PW_FEATURE) {
            double a = phase[i];
            for (int r = 0; r < R; ++r)
                a = fma(Bt[i + (int64_t)r * ldb], qs[r * PW_LANES + lane], a);
            double sn, cn;
            sincos(a, &sn, &cn);
            bv = cn;
            gv = -sn;
        }
        else {
            double z = 0.0;
            for (int r = 0; r < R; ++r) {
                const double d = qs[r * PW_LANES + lane] - Bt[i + (int64_t)r * ldb];
                z = fma(d, d, z);
            }
            bv = kfun_fast_rt(kp.kind, z, kp.sf2);
            gv = RT > 0 ? kgrad_fast_rt(kp.kind, z, kp.sf2) : 0.0;
        }
        double f[RTT];
        if (RT > 0) {
#pragma unroll
            for (int a = 0; a < RTT; ++a) {
                const double x = brow[a][i];
                f[a] = MODE == PW_FEATURE ? x : qr[a] - x;
            }
        }
#pragma unroll
        for (int b = 0; b < CT; ++b) {
            const double w = ccol[b][i];
            acc[b] = fma(bv, w, acc[b]);
            if (RT > 0) {
                const double gw = gv * w;
#pragma unroll
                for (int a = 0; a < RTT; ++a)
                    g[a][b] = fma(gw, f[a], g[a][b]);
            }
        }
    }
    if (m < M)
#pragma unroll
        for (int b = 0; b < CT; ++b) {
            if (c0 + b >= ncol)
                continue;
            double* p = part + ((seg * ncol + c0 + b) * NS) * ldp + m;
            if (r0 == 0)
                p[0] = acc[b];
            if (RT > 0)
#pragma unroll
                for (int a = 0; a < RTT; ++a)
                    if (r0 + a < R)
                        p[(int64_t)(1 + r0 + a) * ldp] = g[a][b];
        }
}

// dst[r ldd + i] = src[r lds + i] s_r: the samples as the data term reads them (the product k_query_grad forms when it stages a sample)
__global__ __launch_bounds__(256) void k_paths_scale_rows(const double* __restrict__ src, int64_t lds, double* __restrict__ dst, int64_t ldd,
                                                          int64_t n, KParams kp)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int r = blockIdx.y;
    if (i < n)
        dst[(int64_t)r * ldd + i] = src[(int64_t)r * lds + i] * kp.inv_ell[r];
}

// F[m + ldf c] = (mean[m + ldm (c / S)] + feature term) + data term, each term its segments' partials added in ascending order;
// dF[m + ldo (d + Din c)] = s_d u[d] + sum_j Lambda[d, j] u[Din + j],  u[row] = feature partials + data partials  (F, dF: either may
// be null; NS = 1 without gradient slots)
__global__ __launch_bounds__(256) void k_paths_fold(const double* __restrict__ partF, int nsegF, const double* __restrict__ partK, int nsegK,
                                                    int64_t ldp, int NS, int ncol, int64_t M, KParams kp, LamParams lp,
                                                    const double* __restrict__ mean, int64_t ldm, int S, double* __restrict__ F, int64_t ldf,
                                                    double* __restrict__ dF, int64_t ldo)
{
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y, R = kp.D, Din = kp.Din, k = kp.k_lam;
    if (m >= M)
        return;
    auto u = [&](int slot) {
        double a = 0.0, b = 0.0;
        for (int seg = 0; seg < nsegF; ++seg)
            a += partF[(((int64_t)seg * ncol + c) * NS + slot) * ldp + m];
        for (int seg = 0; seg < nsegK; ++seg)
            b += partK[(((int64_t)seg * ncol + c) * NS + slot) * ldp + m];
        return slot == 0 ? ((mean ? mean[m + ldm * (c / S)] : 0.0) + a) + b : a + b;
    };
    if (F)
        F[m + ldf * c] = u(0);
    if (!dF || NS != 1 + R)
        return;
    double up[8]; // k <= 7 (qgrad.hip)
#pragma unroll
    for (int j = 0; j < 8; ++j)
        up[j] = j < k ? u(1 + Din + j) : 0.0;
    for (int d = 0; d < Din; ++d) {
        double v = kp.inv_ell[d] * u(1 + d);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < k)
                v = fma(lp.A[d + j * Din], up[j], v);
        dF[m + ldo * (d + (int64_t)Din * c)] = v;
    }
}

// the right-hand sides of the set's solve, transposed (a draw per row, in the place of the query's Kst):
//   Rt[c + ldr (i0 + i)] = om[i0 + i + ldom (c / S)] - (Phi(X) W)[i0 + i, c] - sn E[i0 + i + lde c]      for the n samples from i0 on
__global__ __launch_bounds__(256) void k_paths_residual(const double* __restrict__ partF, int nsegF, int64_t ldp, int ncol, int64_t n,
                                                        int64_t i0, const double* __restrict__ om, int64_t ldom, int S, int c_first,
                                                        const double* __restrict__ E, int64_t lde, double sn, double* __restrict__ Rt,
                                                        int64_t ldr)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    if (i >= n)
        return;
    double a = 0.0;
    for (int seg = 0; seg < nsegF; ++seg)
        a += partF[((int64_t)seg * ncol + c) * ldp + i];
    double r = om[i0 + i + ldom * ((c_first + c) / S)] - a;
    if (E)
        r = fma(-sn, E[i0 + i + lde * c], r);
    Rt[c + ldr * (i0 + i)] = r;
}

// U[i + ldu c] = Wt[c + ldw i]
__global__ __launch_bounds__(256) void k_paths_untranspose(const double* __restrict__ Wt, int64_t ldw, int64_t n, int ncol,
                                                           double* __restrict__ U, int64_t ldu)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n)
        U[i + ldu * blockIdx.y] = Wt[blockIdx.y + ldw * i];
}

// run[2 c], run[2 c + 1] (the bits of an int64): the maximum of column c over the points seen so far and its index; this chunk's
// points are t0 .. t0 + M.  The lowest index on exact ties: chunks arrive in ascending order and only a greater value replaces.
__global__ __launch_bounds__(256) void k_paths_argmax(const double* __restrict__ F, int64_t ldf, int64_t M, int64_t t0, int first,
                                                      double* __restrict__ run)
{
    __shared__ double sv[256];
    __shared__ long long si[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    double bv = -__builtin_inf();
    long long bi = -1;
    for (int64_t m = tid; m < M; m += 256) { // (ascending per thread: the first maximiser stays)
        const double v = F[m + ldf * c];
        if (bi < 0 || v > bv)
            bv = v, bi = m;
    }
    sv[tid] = bv;
    si[tid] = bi;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            const double v = sv[tid + h];
            const long long j = si[tid + h];
            if (j >= 0 && (si[tid] < 0 || v > sv[tid] || (v == sv[tid] && j < si[tid])))
                sv[tid] = v, si[tid] = j;
        }
        __syncthreads();
    }
    if (tid == 0 && si[0] >= 0) {
        if (first || sv[0] > run[2 * c]) {
            run[2 * c] = sv[0];
            const long long idx = t0 + si[0];
            reinterpret_cast<long long*>(run)[2 * c + 1] = idx;
        }
    }
}

// slots per (segment, column) of `part`
int paths_slots(bool grad, int R) { return grad ? 1 + R : 1; }

// one pass: mode 0 the feature term (Bt = Omega0 rows, NB = R features, Cf = amp W), mode 1 the data term (Bt = the scaled samples, Cf = U);
// grad: with the gradient slots.  Tiles from R and grad alone, never from M.
void launch_paths_basis(hipStream_t s, int mode, bool grad, const double* Qt, int64_t ldq, int64_t M, const double* Bt, int64_t ldb, int64_t NB,
                        const double* phase, const double* Cf, int64_t ldc, int ncol, const KParams& kp, int nseg, double* part, int64_t ldp)
{
    if (M <= 0 || ncol <= 0 || NB <= 0)
        return;
    const int R = kp.D;
    // the value alone: sixteen columns per tile from nine columns on — one sincos / exp serves them all, and it is most of the pass
    const int RT = !grad ? 0 : R <= 8 ? 8 : 16, CT = RT == 16 ? 4 : (RT == 0 && ncol > 8) ? 16 : 8;
    const int tiles = (RT ? (R + RT - 1) / RT : 1) * ((ncol + CT - 1) / CT);
    const dim3 grid((unsigned)((M + PW_LANES - 1) / PW_LANES), (unsigned)nseg, (unsigned)tiles), block(PW_LANES);
    const size_t lds = sizeof(double) * (size_t)(R * PW_LANES);
#define PW_GO(md, rt, ct) \
    GPE_LAUNCH((k_paths_basis<md, rt, ct>), grid, block, lds, s, Qt, ldq, M, Bt, ldb, NB, phase, Cf, ldc, ncol, kp, part, ldp)
    if (mode == PW_FEATURE) {
        if (RT == 0 && CT == 16)
            PW_GO(PW_FEATURE, 0, 16);
        else if (RT == 0)
            PW_GO(PW_FEATURE, 0, 8);
        else if (RT == 8)
            PW_GO(PW_FEATURE, 8, 8);
        else
            PW_GO(PW_FEATURE, 16, 4);
    }
    else {
        if (RT == 0 && CT == 16)
            PW_GO(PW_KERNEL, 0, 16);
        else if (RT == 0)
            PW_GO(PW_KERNEL, 0, 8);
        else if (RT == 8)
            PW_GO(PW_KERNEL, 8, 8);
        else
            PW_GO(PW_KERNEL, 16, 4);
    }
#undef PW_GO
}

void launch_paths_scale_rows(hipStream_t s, const double* src, int64_t lds, double* dst, int64_t ldd, int64_t n, const KParams& kp)
{
    if (n <= 0)
        return;
    GPE_LAUNCH(k_paths_scale_rows, dim3((unsigned)((n + 255) / 256), (unsigned)kp.D), dim3(256), 0, s, src, lds, dst, ldd, n, kp);
}

void launch_paths_fold(hipStream_t s, const double* partF, int nsegF, const double* partK, int nsegK, int64_t ldp, int NS, int ncol, int64_t M,
                       const KParams& kp, const LamParams& lp, const double* mean, int64_t ldm, int S, double* F, int64_t ldf, double* dF,
                       int64_t ldo)
{
    if (M <= 0 || ncol <= 0)
        return;
    GPE_LAUNCH(k_paths_fold, dim3((unsigned)((M + 255) / 256), (unsigned)ncol), dim3(256), 0, s, partF, nsegF, partK, nsegK, ldp, NS, ncol, M,
               kp, lp, mean, ldm, S, F, ldf, dF, ldo);
}

void launch_paths_residual(hipStream_t s, const double* partF, int nsegF, int64_t ldp, int ncol, int64_t n, int64_t i0, const double* om,
                           int64_t ldom, int S, int c_first, const double* E, int64_t lde, double sn, double* Rt, int64_t ldr)
{
    if (n <= 0 || ncol <= 0)
        return;
    GPE_LAUNCH(k_paths_residual, dim3((unsigned)((n + 255) / 256), (unsigned)ncol), dim3(256), 0, s, partF, nsegF, ldp, ncol, n, i0, om, ldom,
               S, c_first, E, lde, sn, Rt, ldr);
}

void launch_paths_untranspose(hipStream_t s, const double* Wt, int64_t ldw, int64_t n, int ncol, double* U, int64_t ldu)
{
    if (n <= 0 || ncol <= 0)
        return;
    GPE_LAUNCH(k_paths_untranspose, dim3((unsigned)((n + 255) / 256), (unsigned)ncol), dim3(256), 0, s, Wt, ldw, n, ncol, U, ldu);
}

void launch_paths_argmax(hipStream_t s, const double* F, int64_t ldf, int64_t M, int ncol, int64_t t0, bool first, double* run)
{
    if (M <= 0 || ncol <= 0)
        return;
    GPE_LAUNCH(k_paths_argmax, dim3((unsigned)ncol), dim3(256), 0, s, F, ldf, M, t0, first ? 1 : 0, run);
}
