// grad.hip — gradient of the log marginal likelihood wrt the kernel hyper-parameters (gfx950).
//
// Replaces GP::compute_kernel_grad_log_lik (src/limbo/model/gp.hpp:285-311), which walks the
// N(N+1)/2 pairs calling Kernel::grad (kernel.hpp:86-96; squared_exp_ard.hpp:127-135,
// matern_five_halves.hpp:115-133, matern_three_halves.hpp:109-121, exp.hpp:104-113) and
// allocating a VectorXd per pair:
//     grad_t = sum_{i>j} w_ij g_ij,t + 1/2 sum_i w_ii g_ii,t ,   w = alpha alpha^T - K^-1.
// Here dK/dtheta is never materialised: each 64x64 lower-triangle tile recomputes the pair
// distances from the two sample panels (LDS), reads K^-1 once (coalesced, HBM-read bound:
// N(N+1)/2 * 8 B), and keeps T partial sums in registers.  Partials are written per tile and
// summed in a fixed order by a second kernel, so the result is run-to-run deterministic.
//
// The same pair sum serves the leave-one-out gradient (gp.hpp:354-402).  The reference forms, per
// hyper-parameter j, Zeta_j = K^-1 dK_j, Zeta_j alpha and diag(Zeta_j K^-1) — 2 T dense N^3 products.
// Both terms of gp.hpp:389 are linear in dK_j, so they collapse to ONE weight matrix shared by all j:
//     dLOO/dtheta_j = sum_ab dK_j[a,b] W[a,b],
//     W = sum_p sym(u_p alpha_p^T) - K^-1 diag(c) K^-1,   u_p = K^-1 (alpha_p / kappa),
//     kappa_i = (K^-1)_ii,  c_i = sum_p 1/2 (1 + alpha_ip^2 / kappa_i) / kappa_i
// i.e. one symmetric N^3 product (MFMA GEMM, gemm.hip) + this kernel with (u, alpha, M) in place of
// (alpha, alpha, K^-1) and a factor 2 (the pair sum visits the lower triangle once).
#include "dev.h"
#include "kfun_fast.h" // exp(-h), h >= 0, branch-free (< 1 ulp): the pair loop is arithmetic-bound, libm's exp was a third of it

#define TILE 64

// LAM = false: the length-scale / sigma_f / noise entries (n_theta = number of those without the noise).
// LAM = true : the Din entries of column `lam_col` of Lambda (squared_exp_ard.hpp:118-121):
//              g = -((x1-x2)^T Lambda_col) (x1-x2) k;  n_theta = Din, optimize_noise = 0.
// (Round 6, after the kernel-matrix build: the pair loop runs over DMAX dimensions and PM outputs WITHOUT conditions — the padded ones
// are zeros in registers and in LDS and add exact zeros, same sums bit for bit —, 1 / ell_d sits in registers, and tiles strictly
// below the diagonal take a loop without the triangle's tests; DMAX 2 and 6 and PM = 1 (one output: config 2) are instantiated.
// N = 4096, D = 6: 102 -> see profiles/r06_grad_tiles.log.)
template <int DMAX, bool LAM, int PM>
__global__ __launch_bounds__(256) void k_grad_tiles(const double* __restrict__ Xt, int64_t ldx, int64_t N, KParams kp_,
                                                    const double* __restrict__ Kinv, int64_t ldk,
                                                    const double* __restrict__ alpha, int64_t lda,
                                                    const double* __restrict__ uvec, int P, double kinv_scale,
                                                    int n_theta, int optimize_noise, int lam_col,
                                                    double* __restrict__ partial, const BatchTab* bt)
{
    if (bt) { // batched launch (gridDim.z GPs, dev.h): this GP's buffers and kernel parameters
        const int z = (int)blockIdx.z;
        Xt = bt_rebase(bt, z, Xt);
        Kinv = bt_rebase(bt, z, Kinv);
        alpha = bt_rebase(bt, z, alpha);
        uvec = bt_rebase(bt, z, uvec);
        partial = bt_rebase(bt, z, partial);
    }
    const KParams& kp = bt ? bt->kp[blockIdx.z] : kp_;
    // weight of pair (i, j):  w = 1/2 sum_p (u_ip alpha_jp + alpha_ip u_jp) - Kinv[i, j]
    // (uvec == alpha for the log-likelihood gradient: w = sum_p alpha_ip alpha_jp - K^-1_ij)
    extern __shared__ __attribute__((aligned(16))) double smem[]; // xj[D][64] | aj[P][64] | uj[P][64] | red[4][T]
    const int D = kp.D;
    const int T = n_theta + (optimize_noise ? 1 : 0);
    double* xj = smem;
    double* aj = smem + DMAX * TILE;
    double* uj = aj + PM * TILE;
    double* red = uj + PM * TILE;

    long long b = blockIdx.x;
    long long t = (long long)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
    while ((t + 1) * (t + 2) / 2 <= b)
        ++t;
    while (t * (t + 1) / 2 > b)
        --t;
    const int ti = (int)t, tj = (int)(b - t * (t + 1) / 2);
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t i = (int64_t)ti * TILE + tx;
    const int64_t j0 = (int64_t)tj * TILE;

    const int xrows = LAM ? (D > DMAX ? D : DMAX) : DMAX; // (LAM reads the projection row lrow >= Din as well: all D rows are staged)
    for (int e = threadIdx.x; e < xrows * TILE; e += 256) {
        const int d = e >> 6, c = e & 63;
        xj[e] = (d < D && j0 + c < N) ? Xt[(int64_t)d * ldx + j0 + c] : 0.0;
    }
    for (int e = threadIdx.x; e < PM * TILE; e += 256) {
        const int p = e >> 6, c = e & 63;
        aj[e] = (p < P && j0 + c < N) ? alpha[(int64_t)p * lda + j0 + c] : 0.0;
        uj[e] = (p < P && j0 + c < N) ? 0.5 * uvec[(int64_t)p * lda + j0 + c] : 0.0;
    }
    double xi[DMAX], ie[DMAX], ai[PM], ui[PM];
#pragma unroll
    for (int d = 0; d < DMAX; ++d) {
        xi[d] = (d < D && i < N) ? Xt[(int64_t)d * ldx + i] : 0.0;
        ie[d] = d < D ? kp.inv_ell[d] : 0.0;
    }
#pragma unroll
    for (int p = 0; p < PM; ++p)
        ai[p] = (p < P && i < N) ? alpha[(int64_t)p * lda + i] : 0.0;
#pragma unroll
    for (int p = 0; p < PM; ++p)
        ui[p] = (p < P && i < N) ? 0.5 * uvec[(int64_t)p * lda + i] : 0.0;
    double acc[DMAX + 2];
#pragma unroll
    for (int q = 0; q < DMAX + 2; ++q)
        acc[q] = 0.0;
    const int lrow = kp.Din + lam_col; // LAM: the projection row of this Lambda column
    const double fi = (LAM && i < N) ? Xt[(int64_t)lrow * ldx + i] : 0.0;
    __syncthreads();

    // a tile strictly below the diagonal with all its rows and columns inside N: no tests in the pair loop
    const bool interior_tile = ti > tj && (int64_t)(ti + 1) * TILE <= N;
    auto pairs = [&](auto interior_c) {
        constexpr bool INTERIOR = decltype(interior_c)::value;
#pragma unroll 2
        for (int c = 0; c < 16; ++c) {
            const int cc = ty * 16 + c;
            const int64_t j = j0 + cc;
            if (!INTERIOR && (j >= N || j > i))
                break;
            double w = 0.0; // gp.hpp:293-296
#pragma unroll
            for (int p = 0; p < PM; ++p)
                w = fma(ai[p], uj[p * TILE + cc], fma(ui[p], aj[p * TILE + cc], w));
            w = fma(-kinv_scale, Kinv[i + j * ldk], w); // 0 for the 2nd.. chunk of outputs when P > GPE_MAX_P
            if (!INTERIOR && i == j)
                w *= 0.5; // gp.hpp:303-304
            double z[DMAX];
            double zs = 0.0;
#pragma unroll
            for (int d = 0; d < DMAX; ++d) {
                const double dd = xi[d] - xj[d * TILE + cc]; // (a padded dimension: 0 - 0)
                const double q = dd * ie[d];
                z[d] = LAM ? dd : q * q;
                zs += q * q;
            }
            if (LAM) { // squared_exp_ard.hpp:118-121
                const double k = kp.sf2 * exp_nonpos(-0.5 * zs);
                const double wkf = -(w * k) * (fi - xj[lrow * TILE + cc]);
#pragma unroll
                for (int d = 0; d < DMAX; ++d)
                    acc[d] = fma(wkf, z[d], acc[d]);
            }
            else if (kp.kind == 0) { // squared_exp_ard.hpp:127-135 (k = 0 branch; k > 0: :114-116, :123)
                const double k = kp.sf2 * exp_nonpos(-0.5 * zs);
                const double wk = w * k;
#pragma unroll
                for (int d = 0; d < DMAX; ++d)
                    acc[d] = fma(wk, z[d], acc[d]);
                acc[DMAX] = fma(wk, 2.0, acc[DMAX]);
            }
            else if (kp.kind == 1) { // matern_five_halves.hpp:115-133
                const double r_ = sqrt(zs);
                const double term1 = 2.23606797749978969641 * r_;
                const double term2 = (5.0 / 3.0) * zs;
                const double r = exp_nonpos(-term1);
                const double g0 = kp.sf2 * (r * term1 * (1 + term1 + term2) + (-term1 - 2. * term2) * r);
                const double g1 = 2 * kp.sf2 * (1 + term1 + term2) * r;
                acc[0] = fma(w, g0, acc[0]);
                acc[1] = fma(w, g1, acc[1]);
            }
            else if (kp.kind == 2) { // matern_three_halves.hpp:109-121
                const double term = 1.73205080756887729353 * sqrt(zs);
                const double r = exp_nonpos(-term);
                const double g0 = kp.sf2 * (-term * r + (1 + term) * term * r);
                const double g1 = 2 * kp.sf2 * (1 + term) * r;
                acc[0] = fma(w, g0, acc[0]);
                acc[1] = fma(w, g1, acc[1]);
            }
            else { // exp.hpp:104-113
                const double k = kp.sf2 * exp_nonpos(-0.5 * zs);
                acc[0] = fma(w * k, zs, acc[0]);
                acc[1] = fma(w * k, 2.0, acc[1]);
            }
            if (!INTERIOR && i == j) // kernel.hpp:90-93: 2 * noise on the diagonal
                acc[DMAX + 1] = fma(w, 2.0 * kp.noise, acc[DMAX + 1]);
        }
    };
    if (interior_tile)
        pairs(std::true_type{});
    else if (i < N)
        pairs(std::false_type{});
    // block reduction of the T sums: wave shuffles, then 4 waves through LDS in fixed order
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < DMAX + 2; ++q) {
        double v = acc[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            v += __shfl_down(v, o);
        if (lane == 0)
            red[wv * (DMAX + 2) + q] = v;
    }
    __syncthreads();
    if (threadIdx.x < T) {
        // map output slot -> accumulator slot
        int q;
        if (LAM)
            q = (int)threadIdx.x;
        else if (optimize_noise && (int)threadIdx.x == T - 1)
            q = DMAX + 1;
        else if (kp.kind == 0)
            q = ((int)threadIdx.x == n_theta - 1) ? DMAX : (int)threadIdx.x;
        else
            q = (int)threadIdx.x;
        partial[(int64_t)blockIdx.x * T + threadIdx.x] = red[0 * (DMAX + 2) + q] + red[1 * (DMAX + 2) + q]
            + red[2 * (DMAX + 2) + q] + red[3 * (DMAX + 2) + q];
    }
}

// slot t of the launch goes to grad[out_off + t], slots >= tail_from to grad[tail_to + (t - tail_from)]
// (with Lambda columns the parameter vector is [ell | Lambda columns | sigma_f | (noise)])
__global__ __launch_bounds__(256) void k_grad_final(const double* __restrict__ partial, int64_t nblk, int T,
                                                    double* __restrict__ grad_, int accumulate, int out_off,
                                                    int tail_from, int tail_to, const BatchTab* bt)
{
    BT_REBASE(bt, partial);
    BT_REBASE(bt, grad_);
    __shared__ double sh[4];
    const int t = blockIdx.x;
    double* grad = grad_ + ((t >= tail_from) ? tail_to - tail_from : out_off);
    double s = 0.0;
    for (int64_t b = threadIdx.x; b < nblk; b += 256)
        s += partial[b * T + t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        s += __shfl_down(s, o);
    if ((threadIdx.x & 63) == 0)
        sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0)
        grad[t] = (accumulate ? grad[t] : 0.0) + (sh[0] + sh[1] + sh[2] + sh[3]);
}

static void launch_grad_chunk(hipStream_t s, const double* Xt, int64_t ldx, int64_t N, const KParams& kp,
                              const double* Kinv, int64_t ldk, const double* alpha, int64_t lda, const double* uvec,
                              int P, double kinv_scale, int n_theta, int optimize_noise, int lam_col, double* partial,
                              double* grad, int accumulate, int out_off, int tail_from, int tail_to);

int64_t grad_partial_size(int64_t N, int T)
{
    int64_t nt = (N + TILE - 1) / TILE;
    return nt * (nt + 1) / 2 * T;
}

void launch_grad_loglik(hipStream_t s, const double* Xt, int64_t ldx, int64_t N, const KParams& kp, const double* Kinv,
                        int64_t ldk, const double* alpha, int64_t lda, const double* uvec, int P, int n_theta,
                        int optimize_noise, double* partial, double* grad)
{
    // outputs go through in chunks of GPE_MAX_P: the alpha-u term is additive over outputs, K^-1 enters once
    for (int p0 = 0; p0 < P; p0 += GPE_MAX_P) {
        const int pc = (P - p0 < GPE_MAX_P) ? P - p0 : GPE_MAX_P;
        const double ks = p0 == 0 ? 1.0 : 0.0;
        const double *al = alpha + (int64_t)p0 * lda, *uv = uvec + (int64_t)p0 * lda;
        if (kp.k_lam == 0) {
            launch_grad_chunk(s, Xt, ldx, N, kp, Kinv, ldk, al, lda, uv, pc, ks, n_theta, optimize_noise, -1, partial,
                              grad, p0 > 0, 0, 1 << 30, 0);
            continue;
        }
        // [ell_1..ell_Din | sigma_f | (noise)] -> slots [0, Din) and [n_theta - 1, ...)
        launch_grad_chunk(s, Xt, ldx, N, kp, Kinv, ldk, al, lda, uv, pc, ks, kp.Din + 1, optimize_noise, -1, partial,
                          grad, p0 > 0, 0, kp.Din, n_theta - 1);
        for (int j = 0; j < kp.k_lam; ++j) // one pass per Lambda column: the pair loop is K^-1-read bound, k is small
            launch_grad_chunk(s, Xt, ldx, N, kp, Kinv, ldk, al, lda, uv, pc, ks, kp.Din, 0, j, partial, grad, p0 > 0,
                              kp.Din * (j + 1), 1 << 30, 0);
    }
}

static void launch_grad_chunk(hipStream_t s, const double* Xt, int64_t ldx, int64_t N, const KParams& kp,
                              const double* Kinv, int64_t ldk, const double* alpha, int64_t lda, const double* uvec,
                              int P, double kinv_scale, int n_theta, int optimize_noise, int lam_col, double* partial,
                              double* grad, int accumulate, int out_off, int tail_from, int tail_to)
{
    const int T = n_theta + (optimize_noise ? 1 : 0);
    const int64_t nt = (N + TILE - 1) / TILE;
    const int64_t nblk = nt * (nt + 1) / 2;
    const int D = kp.D;
    dim3 grid((unsigned)nblk, 1, (unsigned)g_batch.G), block(256);
#define LG(DM, LAM, PMV)                                                                                         \
    GPE_LAUNCH((k_grad_tiles<DM, LAM, PMV>), grid, block,                                                        \
                       (size_t)(((LAM) && D > DM ? D : DM) * TILE + 2 * PMV * TILE + 4 * (DM + 2)) * sizeof(double), s, Xt, ldx, N, \
                       kp, Kinv, ldk, alpha, lda, uvec, P, kinv_scale, n_theta, optimize_noise, lam_col, partial, g_batch.bt)
#define LGP(DM)                   \
    do {                          \
        if (P == 1)               \
            LG(DM, false, 1);     \
        else                      \
            LG(DM, false, GPE_MAX_P); \
    } while (0)
    if (lam_col >= 0) {
        if (D <= 4)
            LG(4, true, GPE_MAX_P);
        else if (D <= 8)
            LG(8, true, GPE_MAX_P);
        else if (D <= 16)
            LG(16, true, GPE_MAX_P);
        else if (D <= 32)
            LG(32, true, GPE_MAX_P);
        else
            LG(64, true, GPE_MAX_P);
    }
    else {
        if (D <= 2)
            LGP(2);
        else if (D <= 4)
            LGP(4);
        else if (D <= 6)
            LGP(6);
        else if (D <= 8)
            LGP(8);
        else if (D <= 16)
            LGP(16);
        else if (D <= 32)
            LGP(32);
        else
            LGP(64);
    }
#undef LGP
#undef LG
    GPE_LAUNCH(k_grad_final, dim3((unsigned)T, 1, (unsigned)g_batch.G), dim3(256), 0, s, partial, nblk, T, grad, accumulate,
                       out_off, tail_from, tail_to, g_batch.bt);
}

// ---- leave-one-out helpers (gp.hpp:339-402) -------------------------------------------------------
// per sample i: kappa = (K^-1)_ii;  v[i, p] = alpha[i, p] / kappa;  sc[i] = sqrt(c_i);
// val[i] = sum_p (-1/2 alpha_ip^2 / kappa + 1/2 log kappa - 1/2 log 2 pi)        (gp.hpp:348)
__global__ __launch_bounds__(256) void k_loo_prep(const double* __restrict__ Kinv, int64_t ldk, int64_t N,
                                                  const double* __restrict__ alpha, int64_t lda, int P,
                                                  double* __restrict__ v, double* __restrict__ sc,
                                                  double* __restrict__ val)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N)
        return;
    const double kappa = Kinv[i + i * ldk];
    const double inv_d = 1.0 / kappa;
    double c = 0.0, l = 0.0;
    for (int p = 0; p < P; ++p) {
        const double a = alpha[i + (int64_t)p * lda];
        if (v)
            v[i + (int64_t)p * lda] = a * inv_d;
        c += 0.5 * (1.0 + a * a * inv_d) * inv_d;
        l += -0.5 * a * a * inv_d - 0.5 * log(inv_d) - 0.9189385332046727418; // 1/2 log(2 pi)
    }
    if (sc)
        sc[i] = sqrt(c);
    val[i] = l;
}
// out[0] = sum_i val[i], fixed order (one workgroup)
__global__ __launch_bounds__(256) void k_sum_fixed(const double* __restrict__ val, int64_t N, double* __restrict__ out)
{
    __shared__ double sh[4];
    double s = 0.0;
    for (int64_t b = threadIdx.x; b < N; b += 256)
        s += val[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        s += __shfl_down(s, o);
    if ((threadIdx.x & 63) == 0)
        sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0)
        out[0] = sh[0] + sh[1] + sh[2] + sh[3];
}
// S = sym(Kl) diag(sc): S[i, j] = K^-1[i, j] sc[j] for the full square, Kl holding the lower triangle
__global__ __launch_bounds__(256) void k_sym_colscale(const double* __restrict__ Kl, int64_t ldk, int64_t N,
                                                      const double* __restrict__ sc, double* __restrict__ S,
                                                      int64_t lds_)
{
    __shared__ double tile[TILE][TILE + 1];
    const int ti = blockIdx.y, tj = blockIdx.x; // lower-triangle tiles only
    if (tj > ti)
        return;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)ti * TILE, j0 = (int64_t)tj * TILE;
    for (int c = ty; c < TILE; c += 4) {
        const int64_t i = i0 + tx, j = j0 + c;
        double kv = 0.0;
        if (i < N && j < N)
            kv = (j <= i) ? Kl[i + j * ldk] : Kl[j + i * ldk];
        tile[c][tx] = kv;
        if (i < N && j < N)
            S[i + j * lds_] = kv * sc[j];
    }
    __syncthreads();
    if (ti == tj)
        return;
    for (int c = ty; c < TILE; c += 4) { // mirrored tile: S[j, i] = K^-1[i, j] sc[i]
        const int64_t jj = j0 + tx, ii = i0 + c;
        if (jj < N && ii < N)
            S[jj + ii * lds_] = tile[tx][c] * sc[ii];
    }
}
__global__ void k_scale_vec(double* __restrict__ g, int n, double f)
{
    // (n = n_theta + noise reaches GPE_MAX_THETA + 1 = 65, one more than the wave: with `if (threadIdx.x < n)` the LOO
    // gradient's noise entry stayed unscaled, half its value, at 64 parameters with optimize_noise)
    for (int t = (int)threadIdx.x; t < n; t += (int)blockDim.x)
        g[t] *= f;
}

void launch_loo_prep(hipStream_t s, const double* Kinv, int64_t ldk, int64_t N, const double* alpha, int64_t lda, int P,
                     double* v, double* sc, double* val, double* out)
{
    GPE_LAUNCH(k_loo_prep, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, Kinv, ldk, N, alpha, lda, P, v,
                       sc, val);
    GPE_LAUNCH(k_sum_fixed, dim3(1), dim3(256), 0, s, val, N, out);
}
void launch_sym_colscale(hipStream_t s, const double* Kl, int64_t ldk, int64_t N, const double* sc, double* S,
                         int64_t lds_)
{
    const unsigned nt = (unsigned)((N + TILE - 1) / TILE);
    GPE_LAUNCH(k_sym_colscale, dim3(nt, nt), dim3(256), 0, s, Kl, ldk, N, sc, S, lds_);
}
void launch_scale_vec(hipStream_t s, double* g, int n, double f)
{
    GPE_LAUNCH(k_scale_vec, dim3(1), dim3(64), 0, s, g, n, f);
}
