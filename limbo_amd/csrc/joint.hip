// joint.hip — the joint posterior over a batch of M query points (include/gpe_joint.h): covariance, draws, arg-max.
//
//   Sigma = K(V, V) + jitter I - Zt Zt^T          Zt[m + i ldz] = (L^-1 k(X, v_m))_i, the transposed layout of query.hpp
//   F     = mean_q + kta + C Z                    C = chol(Sigma), lower; Z standard normals supplied by the caller
//
// The product Zt Zt^T has a LONG k (= N, 4096 .. 16 384) and FEW tiles (M = 1024: 36 lower 128 x 128 tiles for 256 CUs), so its
// k range is split over workgroups: one workgroup per (lower tile, k chunk) runs the direct-to-LDS matrix-core tile product of
// the engine's tile lists (gemm.hip: k_gemm_items — both operands are contiguous along m in the transposed layout) and leaves
// its partial tile in partial matrix `chunk`; a second launch (k_cov_fold, here) adds a tile's partials in ascending k — a
// fixed order, no floating-point atomics, no arrival counters: bitwise reproducible whatever CUs were free — generates
// k(v_a, v_b) (+ jitter on the diagonal), and stores the tile together with its mirror, so Sigma is written once.
#include <algorithm>
#include <vector>

#include "dev.h"

namespace {
constexpr int CT = 128;     // tile edge of the covariance product
constexpr int KSTEP = 16;   // k step of k_gemm_items: chunk bounds are multiples of it
constexpr int KMIN = 256;   // no chunk shorter than this (a cut costs a second pass over the tile)
constexpr int NCH_MAX = 256; // partial matrices at most (only a batch of a tile or two gets there)
} // namespace

// how many chunks the k range of every tile is cut into: enough workgroups for two per CU, no chunk below KMIN
static int cov_chunks(int64_t M, int64_t N, int cus)
{
    const int64_t nt = (M + CT - 1) / CT, tiles = nt * (nt + 1) / 2;
    const int64_t units = (N + KSTEP - 1) / KSTEP;
    int64_t nch = (2 * (int64_t)cus + tiles - 1) / tiles;
    nch = std::min<int64_t>(nch, std::max<int64_t>(1, units / (KMIN / KSTEP)));
    return (int)std::max<int64_t>(1, std::min<int64_t>(nch, NCH_MAX));
}

int joint_cov_chunks(int64_t M, int64_t N, int cus) { return cov_chunks(M, N, cus); }

// rows of 5: { tile i, tile j (j <= i), k0, k1 (<= N), partial slot }: one workgroup each, in launch order (chunk-major: the
// workgroups in flight together read the same k range of Zt).  Returns the number of rows.
int joint_cov_plan(int64_t M, int64_t N, int cus, int64_t* out, int64_t cap_rows)
{
    if (M <= 0 || N <= 0 || cus <= 0)
        return -1;
    const int64_t nt = (M + CT - 1) / CT;
    const int64_t units = (N + KSTEP - 1) / KSTEP;
    const int nch = cov_chunks(M, N, cus);
    const int64_t base = units / nch, rem = units % nch;
    int64_t row = 0, u0 = 0;
    for (int c = 0; c < nch; ++c) {
        const int64_t u = base + (c < rem ? 1 : 0);
        const int64_t k0 = u0 * KSTEP, k1 = std::min<int64_t>((u0 + u) * KSTEP, N);
        for (int64_t i = 0; i < nt; ++i)
            for (int64_t j = 0; j <= i; ++j, ++row) {
                if (!out || row >= cap_rows)
                    continue;
                int64_t* o = out + row * 5;
                o[0] = i;
                o[1] = j;
                o[2] = k0;
                o[3] = k1;
                o[4] = c;
            }
        u0 += u;
    }
    return (int)row;
}

// Sigma[a, b] = k(v_a, v_b) + jitter [a == b] - sum_c Part_c[a, b], lower tiles, each stored with its mirror.
// One workgroup per lower 128 x 128 tile and 32-column strip of it; thread = (row, 2 column phases).
__global__ __launch_bounds__(256) void k_cov_fold(const double* __restrict__ Part, int64_t ldp, int64_t pstride, int nch,
                                                  const double* __restrict__ Qt, int64_t ldq, int64_t M, KParams kp, double jitter,
                                                  double* __restrict__ Sig, int64_t lds)
{
    // linear tile id -> (ti >= tj)
    const int t = (int)blockIdx.x;
    int ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((ti + 1) * (ti + 2) / 2 <= t)
        ++ti;
    while (ti * (ti + 1) / 2 > t)
        --ti;
    const int tj = t - ti * (ti + 1) / 2;
    const int64_t b0 = (int64_t)tj * CT + (int64_t)blockIdx.y * 32;
    const int D = kp.D;
    const int r = threadIdx.x & 127, half = threadIdx.x >> 7;
    const int64_t a = (int64_t)ti * CT + r;
    if (a >= M)
        return;
    for (int cc = half; cc < 32; cc += 2) {
        const int64_t b = b0 + cc;
        if (b >= M || b > a)
            break; // (columns ascend: nothing further of this row is in the lower triangle)
        double z = 0.0;
        for (int d = 0; d < D; ++d) {
            // the difference is scaled, as k_build does (kbuild.hip): the same z, bit for bit
            const double q = (Qt[(int64_t)d * ldq + a] - Qt[(int64_t)d * ldq + b]) * kp.inv_ell[d];
            z = fma(q, q, z);
        }
        double acc = Part[a + b * ldp];
        for (int c = 1; c < nch; ++c) // ascending k: the fixed order of the reduction
            acc += Part[(int64_t)c * pstride + a + b * ldp];
        double v = kfun(kp.kind, z, kp.sf2);
        if (a == b)
            v += jitter;
        v -= acc;
        Sig[a + b * lds] = v;
        if (a != b)
            Sig[b + a * lds] = v;
    }
}

void launch_cov_fold(hipStream_t s, const double* Part, int64_t ldp, int64_t pstride, int nch, const double* Qt, int64_t ldq, int64_t M,
                     const KParams& kp, double jitter, double* Sig, int64_t lds)
{
    if (M <= 0)
        return;
    const int64_t nt = (M + CT - 1) / CT;
    GPE_LAUNCH(k_cov_fold, dim3((unsigned)(nt * (nt + 1) / 2), CT / 32), dim3(256), 0, s, Part, ldp, pstride, nch, Qt, ldq, M, kp, jitter, Sig,
               lds);
}

// F[m, col] = mean_q[m, p] + kta[m, p] + sum_{j <= m} C[m, j] Z[j, col]   col = s + S p, columns [col0, col0 + nc), nc <= 64.
// One workgroup per 64 rows; thread = (row, column phase of 4): up to 16 columns each.  C is read once per column phase
// (coalesced along m, the other three phases hit the cache), Z through LDS, j ascending: a fixed summation order.
__global__ __launch_bounds__(256) void k_draws(const double* __restrict__ Cm, int64_t ldc, int64_t M, const double* __restrict__ Z,
                                               const double* __restrict__ mean_q, const double* __restrict__ kta, int64_t ldk, int S,
                                               int col0, int nc, double* __restrict__ F)
{
    __shared__ double zs[64][64 + 1]; // [j][col]
    const int r = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * 64, m = m0 + r;
    double acc[16];
#pragma unroll
    for (int q = 0; q < 16; ++q)
        acc[q] = 0.0;
    const int64_t jend = std::min<int64_t>(m0 + 64, M);
    for (int64_t j0 = 0; j0 < jend; j0 += 64) {
        __syncthreads();
        for (int e = threadIdx.x; e < 64 * 64; e += 256) {
            const int jj = e & 63, cc = e >> 6;
            zs[jj][cc] = (cc < nc && j0 + jj < M) ? Z[(j0 + jj) + (int64_t)(col0 + cc) * M] : 0.0;
        }
        __syncthreads();
        if (m < M) {
            const int jn = (int)std::min<int64_t>(64, m - j0 + 1); // j <= m: the lower triangle only
            for (int jj = 0; jj < jn; ++jj) {
                const double cv = Cm[m + (j0 + jj) * ldc];
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    acc[q] = fma(cv, zs[jj][ph + 4 * q], acc[q]);
            }
        }
    }
    if (m >= M)
        return;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int cc = ph + 4 * q;
        if (cc < nc) {
            const int col = col0 + cc, p = col / S;
            double v = kta[m + (int64_t)p * ldk] + acc[q];
            if (mean_q)
                v = mean_q[m + (int64_t)p * M] + v;
            F[m + (int64_t)col * M] = v;
        }
    }
}

void launch_draws(hipStream_t s, const double* Cm, int64_t ldc, int64_t M, const double* Z, const double* mean_q, const double* kta, int64_t ldk,
                  int S, int ncols, double* F)
{
    for (int col0 = 0; col0 < ncols && M > 0; col0 += 64) {
        const int nc = std::min(64, ncols - col0);
        GPE_LAUNCH(k_draws, dim3((unsigned)((M + 63) / 64)), dim3(256), 0, s, Cm, ldc, M, Z, mean_q, kta, ldk, S, col0, nc, F);
    }
}

// per column of F: the largest value and the LOWEST index that holds it.  out[2 col] = value, out[2 col + 1] = the index's bits.
__global__ __launch_bounds__(256) void k_argmax(const double* __restrict__ F, int64_t M, double* __restrict__ out)
{
    __shared__ double sv[256];
    __shared__ long long si[256];
    const double* f = F + (int64_t)blockIdx.x * M;
    double bv = 0.0;
    long long bi = -1;
    for (int64_t m = threadIdx.x; m < M; m += 256) { // ascending m per thread: `>` keeps the lowest index of equal values
        const double v = f[m];
        if (bi < 0 || v > bv) {
            bv = v;
            bi = m;
        }
    }
    sv[threadIdx.x] = bv;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const double ov = sv[threadIdx.x + w];
            const long long oi = si[threadIdx.x + w];
            const long long mi = si[threadIdx.x];
            if (oi >= 0 && (mi < 0 || ov > sv[threadIdx.x] || (ov == sv[threadIdx.x] && oi < mi))) {
                sv[threadIdx.x] = ov;
                si[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = sv[0];
        out[2 * blockIdx.x + 1] = __longlong_as_double(si[0]);
    }
}

void launch_argmax(hipStream_t s, const double* F, int64_t M, int ncols, double* out)
{
    if (ncols > 0 && M > 0)
        GPE_LAUNCH(k_argmax, dim3((unsigned)ncols), dim3(256), 0, s, F, M, out);
}
