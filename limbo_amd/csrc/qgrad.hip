// qgrad.hip — the gradient of the batched posterior in the query point (include/gpe_query_grad.h): one pass over
// Wt = (K^-1 k(X, V))^T and alpha.  Host side: qgrad.hpp.
//
// Every kernel with device code has d k(v, x) / d v = g(z) Mm (v - x), z = (v - x)^T Mm (v - x) (kfun_fast.h computes the value
// from the same z).  With the SoA rows the engine keeps — the D inputs and, for SE-ARD with Lambda, the k projections Lambda^T x,
// R = D + k rows in all — z is a plain sum of squares of s_r (v_r - x_r), s_r = 1 / ell_r (1 on the projection rows), and
//   Mm (v - x) = [ s_d^2 (v_d - x_d) + sum_j Lambda[d, j] (Lambda^T (v - x))_j ]_d.
// So the pass accumulates, per point m and column c, the R-vector  u_c[r] = sum_i C_c[m, i] g(z_mi) s_r (v_mr - x_ir)  in the
// rows as they stand, and the fold kernel applies s_d and Lambda once per point at the end.  The columns: alpha_p (p < P) for
// d(k^T alpha_p) / dv and -2 Wt[m, :] for d var / dv.
#include "dev.h"
#include "kfun_fast.h"

#define QG_LANES 64 // thread = point; one wave per workgroup (LDS per workgroup is small: many workgroups per CU)

// part[((seg ncol + c) R + r) ldp + m] = sum over the samples i of segment seg of  C_c[m, i] g(z_mi) s_r (v_mr - x_ir)
//   grid: x = 64-point groups, y = segments of the samples (gridDim.y of them, equal lengths), z = (row tile, column tile)
//   LDS : qs[R][64] the workgroup's points, xs[R][ch] and as[CT][ch] a stretch of ch samples (ch a multiple of 4), all scaled by s_r
// The thread keeps RT x CT accumulators (rows r0 .. r0 + RT of columns c0 .. c0 + CT) and recomputes z over all R rows: the
// D (P + 1) accumulators of a point do not fit in registers for D up to 62 and any P.
// Column c of the call is cbeg + c; column P is the variance's (coefficient -2 Wt, Wt may be null: the column is then zero).
template <int RT, int CT>
__global__ __launch_bounds__(QG_LANES) void k_query_grad(const double* __restrict__ Qt, int64_t ldq, int64_t M,
                                                         const double* __restrict__ Xt, int64_t ldx, int64_t N,
                                                         const double* __restrict__ Wt, int64_t ldw,
                                                         const double* __restrict__ Al, int64_t lda, int P, KParams kp, int cbeg,
                                                         int ncol, int ch, double* __restrict__ part, int64_t ldp)
{
    extern __shared__ __attribute__((aligned(16))) double qg_lds[];
    const int R = kp.D, lane = threadIdx.x;
    double* qs = qg_lds;           // R x 64
    double* xs = qs + R * QG_LANES; // R x ch
    double* as = xs + R * ch;      // CT x ch
    const int row_tiles = (R + RT - 1) / RT;
    const int r0 = ((int)blockIdx.z % row_tiles) * RT, c0 = ((int)blockIdx.z / row_tiles) * CT;
    const int64_t m = (int64_t)blockIdx.x * QG_LANES + lane, mc = m < M ? m : M - 1;
    const int64_t nseg = gridDim.y, seg = blockIdx.y;
    const int64_t len = (N + nseg - 1) / nseg, i0 = seg * len, i1 = i0 + len < N ? i0 + len : N;

    for (int r = 0; r < R; ++r)
        qs[r * QG_LANES + lane] = Qt[mc + (int64_t)r * ldq] * kp.inv_ell[r];
    double qr[RT], acc[RT][CT], wsel[CT];
#pragma unroll
    for (int a = 0; a < RT; ++a) {
        const int r = r0 + a < R ? r0 + a : R - 1; // (rows beyond R: a copy of the last one, never stored)
        qr[a] = Qt[mc + (int64_t)r * ldq] * kp.inv_ell[r];
#pragma unroll
        for (int b = 0; b < CT; ++b)
            acc[a][b] = 0.0;
    }
#pragma unroll
    for (int b = 0; b < CT; ++b)
        wsel[b] = (Wt && cbeg + c0 + b == P) ? -2.0 : 0.0;
    const bool use_w = Wt && cbeg + c0 <= P && P < cbeg + c0 + CT;

    for (int64_t j0 = i0; j0 < i1; j0 += ch) {
        const int cn = (int)(i1 - j0 < ch ? i1 - j0 : ch);
        __syncthreads();
        // the stretch's samples (beyond cn: zeros, with zero coefficients)
        for (int r = 0; r < R; ++r) { // (r wave-uniform: the scale is a scalar load)
            const double sc = kp.inv_ell[r];
            for (int i = lane; i < ch; i += QG_LANES)
                xs[r * ch + i] = i < cn ? Xt[j0 + i + (int64_t)r * ldx] * sc : 0.0;
        }
        for (int b = 0; b < CT; ++b) {
            const int c = cbeg + c0 + b;
            const bool live = c < P && c0 + b < ncol;
            for (int i = lane; i < ch; i += QG_LANES)
                as[b * ch + i] = (live && i < cn) ? Al[j0 + i + (int64_t)c * lda] : 0.0;
        }
        __syncthreads();
        for (int i = 0; i < cn; i += 4) {
            double z[4] = {0.0, 0.0, 0.0, 0.0}, w[4] = {0.0, 0.0, 0.0, 0.0};
            if (use_w) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { // (clamped address, exact 0 / 1 factor: no conditional load)
                    const int ic = i + j < cn ? i + j : cn - 1;
                    w[j] = Wt[mc + (j0 + ic) * ldw] * (i + j < cn ? 1.0 : 0.0);
                }
            }
            for (int r = 0; r < R; ++r) {
                const double q = qs[r * QG_LANES + lane];
                const double* x = xs + r * ch + i;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double d = q - x[j];
                    z[j] = fma(d, d, z[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double g = kgrad_fast_rt(kp.kind, z[j], kp.sf2);
                double cg[CT];
#pragma unroll
                for (int b = 0; b < CT; ++b)
                    cg[b] = fma(wsel[b], w[j], as[b * ch + i + j]) * g;
#pragma unroll
                for (int a = 0; a < RT; ++a) {
                    const int r = r0 + a < R ? r0 + a : R - 1;
                    const double d = qr[a] - xs[r * ch + i + j];
#pragma unroll
                    for (int b = 0; b < CT; ++b)
                        acc[a][b] = fma(cg[b], d, acc[a][b]);
                }
            }
        }
    }
    if (m < M)
#pragma unroll
        for (int b = 0; b < CT; ++b)
#pragma unroll
            for (int a = 0; a < RT; ++a)
                if (c0 + b < ncol && r0 + a < R)
                    part[((seg * ncol + c0 + b) * R + r0 + a) * ldp + m] = acc[a][b];
}

// out[m + ldo (d + Din c)] = s_d u_c[d] + sum_j Lambda[d, j] u_c[Din + j],  u_c[r] = the segments' partials added in ascending order
__global__ __launch_bounds__(256) void k_query_grad_fold(const double* __restrict__ part, int64_t ldp, int nseg, int ncol, int64_t M,
                                                         KParams kp, LamParams lp, double* __restrict__ out, int64_t ldo)
{
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y, R = kp.D, Din = kp.Din, k = kp.k_lam;
    if (m >= M)
        return;
    auto u = [&](int r) {
        double s = 0.0;
        for (int seg = 0; seg < nseg; ++seg)
            s += part[(((int64_t)seg * ncol + c) * R + r) * ldp + m];
        return s;
    };
    double up[8]; // k <= 7: D + D k + 1 <= GPE_MAX_THETA with k <= D
#pragma unroll
    for (int j = 0; j < 8; ++j)
        up[j] = j < k ? u(Din + j) : 0.0;
    for (int d = 0; d < Din; ++d) {
        double v = kp.inv_ell[d] * u(d);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < k)
                v = fma(lp.A[d + j * Din], up[j], v);
        out[m + ldo * (d + (int64_t)Din * c)] = v;
    }
}

// samples staged per stretch: the workgroup's LDS is (R (64 + ch) + CT ch) doubles, <= 48.3 KiB at R = 63
static int query_grad_stretch(int R) { return R <= 32 ? 64 : 32; }
// doubles of `part` for mc points (ldp >= mc), ncol columns
size_t query_grad_partial_doubles(int nseg, int ncol, int R, int64_t ldp) { return (size_t)nseg * (size_t)ncol * (size_t)R * (size_t)ldp; }

// Columns [cbeg, cbeg + ncol) of { alpha_0 .. alpha_{P-1}, -2 Wt } for the M points Qt (SoA, ldq) against the N samples Xt (SoA,
// ldx): out[m + ldo (d + Din c)], c counted from cbeg.  Wt: M x N (ldw), null when column P is not asked for.
void launch_query_grad(hipStream_t s, const double* Qt, int64_t ldq, int64_t M, const double* Xt, int64_t ldx, int64_t N, const double* Wt,
                       int64_t ldw, const double* Al, int64_t lda, int P, const KParams& kp, const LamParams& lp, int cbeg, int ncol, int nseg,
                       double* part, int64_t ldp, double* out, int64_t ldo)
{
    if (M <= 0 || ncol <= 0 || N <= 0)
        return;
    const int R = kp.D, ch = query_grad_stretch(R);
    const int RT = R <= 8 ? 8 : 16, CT = ncol <= 2 ? 2 : 4;
    const int tiles = ((R + RT - 1) / RT) * ((ncol + CT - 1) / CT);
    const dim3 grid((unsigned)((M + QG_LANES - 1) / QG_LANES), (unsigned)nseg, (unsigned)tiles), block(QG_LANES);
    const size_t lds = sizeof(double) * (size_t)(R * (QG_LANES + ch) + CT * ch);
#define QG_GO(rt, ct)                                                                                                               \
    GPE_LAUNCH((k_query_grad<rt, ct>), grid, block, lds, s, Qt, ldq, M, Xt, ldx, N, Wt, ldw, Al, lda, P, kp, cbeg, ncol, ch, part, ldp)
    if (RT == 8 && CT == 2)
        QG_GO(8, 2);
    else if (RT == 8)
        QG_GO(8, 4);
    else if (CT == 2)
        QG_GO(16, 2);
    else
        QG_GO(16, 4);
#undef QG_GO
    GPE_LAUNCH(k_query_grad_fold, dim3((unsigned)((M + 255) / 256), (unsigned)ncol), dim3(256), 0, s, part, ldp, nseg, ncol, M, kp, lp, out, ldo);
}
