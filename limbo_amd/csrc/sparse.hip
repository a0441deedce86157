// sparse.hip — kernels of the sparse pseudo-input GP (include/gpe_sparse.h; spgp.hpp:394-406): ep, r, the weighted Gram.
//
//   ep_n = 1 + (c - sum_i V[i, n]^2) / sig        w_n = 1 / ep_n                                   (spgp.hpp:399)
//   r    = sum_n V[:, n] w_n y_n                    M x P                                            (:402-403, :406: V y / ep)
//   A    = sum_n w_n V[:, n] V[:, n]^T              M x M, lower 64 x 64 tiles                       (:402, :405: V V^T / ep)
//
// V arrives one chunk of columns at a time in one of the two layouts of the batched query (csrc/query.hpp): transposed,
// Zt[n + i ldq] (n contiguous: the k index of the Gram), or — fewer pseudo-inputs than one outer panel — V[i + n ld].  Every
// kernel here takes the element (n, i) at Z[n sn + i si].
//
// The Gram has FEW tiles (M = 1024: 136 lower 64 x 64 tiles) and an ENORMOUS k (a chunk: 10^4 .. 10^5 columns), and in the
// transposed layout both operands are contiguous along k — not the operand form of the direct-to-LDS kernels (gemm.hip), which
// want the non-k index contiguous.  k_sp_gram: one workgroup per (lower tile, k slice) of the plan (gram_plan, below); 32 columns
// of k at a time go through registers (the next step's loads are in flight under this step's products) into LDS as [row][k]
// with a row stride of 34 doubles — the wave's ds_read_b64 of 16 rows x 2 k per half-wave then touches banks 4 i + 2 k, each
// once (MI355X: 64 banks, 32 lanes per LDS cycle) — the weight multiplied into ONE operand on the way; v_mfma_f64_16x16x4_f64.  A
// slice leaves its partial tile in partial matrix `slot`; k_sp_fold adds a tile's partials in ascending slot = ascending k: a
// fixed order, no floating-point atomics.  With one slice per tile (enough tiles to fill the chip) the kernel adds into A itself.
#include <algorithm>

#include "dev.h"

namespace {
constexpr int GT = 64;        // tile edge
constexpr int GKC = 32;       // k columns per LDS step
constexpr int GLD = GKC + 2;  // LDS row stride in doubles (see above)
constexpr int GKU = 64;       // slice bounds are multiples of this
constexpr int GKMIN = 256;    // no slice shorter (a cut costs a pass over the tile)
constexpr int GSL_MAX = 64;   // slices per chunk at most
} // namespace

int64_t sparse_default_chunk(int64_t M)
{
    // the chunk's two M x chunk buffers (cross kernel / running right-hand side, and V^T) under 2^26 doubles = 512 MiB
    const int64_t c = (((int64_t)1 << 26) / (2 * std::max<int64_t>(M, 1))) / 64 * 64;
    return std::max<int64_t>(256, std::min<int64_t>(c, 65536));
}

int sparse_gram_slices(int64_t M, int64_t len, int cus)
{
    const int64_t nt = (M + GT - 1) / GT, tiles = nt * (nt + 1) / 2;
    int64_t s = (2 * (int64_t)cus + tiles - 1) / tiles;
    s = std::min<int64_t>(s, std::max<int64_t>(1, len / GKMIN));
    s = std::min<int64_t>(s, (len + GKU - 1) / GKU);
    return (int)std::max<int64_t>(1, std::min<int64_t>(s, GSL_MAX));
}

// rows of 5: { tile i, tile j <= i, k0, k1, slot }, chunk by chunk, slice by slice (the workgroups in flight together read the
// same columns of V); slot counts on from chunk to chunk: ascending slot = ascending k0 for every tile
int64_t sparse_gram_plan(int64_t M, int64_t N, int64_t chunk, int cus, int64_t* out, int64_t cap_rows)
{
    if (M <= 0 || N <= 0 || cus <= 0)
        return -1;
    if (chunk <= 0)
        chunk = sparse_default_chunk(M);
    chunk = (chunk + 63) / 64 * 64;
    const int64_t nt = (M + GT - 1) / GT;
    int64_t row = 0, slot0 = 0;
    for (int64_t n0 = 0; n0 < N; n0 += chunk) {
        const int64_t len = std::min<int64_t>(chunk, N - n0);
        const int S = sparse_gram_slices(M, len, cus);
        const int64_t units = (len + GKU - 1) / GKU, base = units / S, rem = units % S;
        int64_t u0 = 0;
        for (int s = 0; s < S; ++s) {
            const int64_t u = base + (s < rem ? 1 : 0);
            const int64_t k0 = n0 + u0 * GKU, k1 = std::min<int64_t>(n0 + (u0 + u) * GKU, n0 + len);
            for (int64_t i = 0; i < nt; ++i)
                for (int64_t j = 0; j <= i; ++j, ++row) {
                    if (!out || row >= cap_rows)
                        continue;
                    int64_t* o = out + row * 5;
                    o[0] = i;
                    o[1] = j;
                    o[2] = k0;
                    o[3] = k1;
                    o[4] = slot0 + s;
                }
            u0 += u;
        }
        slot0 += S;
    }
    return row;
}

// ---- ep, w -----------------------------------------------------------------------------------------------------------
// thread = point n of the chunk; the sum over the M pseudo-inputs runs in ascending i whatever the layout.  One wave per
// workgroup: a chunk of 32 768 points is 512 workgroups, not 128, for the 256 CUs (memory-bound: the chunk of V is read once)
__global__ __launch_bounds__(64) void k_sp_ep(const double* __restrict__ Z, int64_t sn, int64_t si, int64_t nc, int64_t M, double c,
                                               double sig, double* __restrict__ ep, double* __restrict__ w)
{
    const int64_t n = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (n >= nc)
        return;
    const double* z = Z + n * sn;
    double ss = 0.0;
    for (int64_t i = 0; i < M; ++i) {
        const double v = z[i * si];
        ss = fma(v, v, ss);
    }
    const double e = 1.0 + (c - ss) / sig; // spgp.hpp:399
    ep[n] = e;
    w[n] = 1.0 / e;
}

static __device__ __forceinline__ double sp_block_sum(double v, double* sh)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v += __shfl_down(v, o);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0)
        sh[wv] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3]; // fixed order
}

// R[i + p ldr] += sum_n Z[n, i] w_n y[n + p ldy]: workgroup = (pseudo-input i, output p); one workgroup owns an entry, the
// chunks follow each other on the stream: a fixed order
__global__ __launch_bounds__(256) void k_sp_r(const double* __restrict__ Z, int64_t sn, int64_t si, int64_t nc, const double* __restrict__ w,
                                              const double* __restrict__ y, int64_t ldy, double* __restrict__ R, int64_t ldr)
{
    __shared__ double sh[4];
    const int64_t i = blockIdx.x;
    const int p = blockIdx.y;
    const double* z = Z + i * si;
    const double* yp = y + (int64_t)p * ldy;
    double s = 0.0;
    for (int64_t n = threadIdx.x; n < nc; n += 256)
        s = fma(z[n * sn], w[n] * yp[n], s);
    s = sp_block_sum(s, sh);
    if (threadIdx.x == 0)
        R[i + (int64_t)p * ldr] += s;
}

// out[0] = sum_n log ep_n, out[1 + p] = sum_n y[n, p]^2 / ep_n (= yh_p . yh_p): one workgroup, thread t takes n = t, t + 256, ..
__global__ __launch_bounds__(256) void k_sp_sums(const double* __restrict__ ep, int64_t N, const double* __restrict__ y, int64_t ldy, int P,
                                                 double* __restrict__ out)
{
    __shared__ double sh[4];
    double s = 0.0;
    for (int64_t n = threadIdx.x; n < N; n += 256)
        s += log(ep[n]);
    s = sp_block_sum(s, sh);
    if (threadIdx.x == 0)
        out[0] = s;
    for (int p = 0; p < P; ++p) {
        const double* yp = y + (int64_t)p * ldy;
        double a = 0.0;
        for (int64_t n = threadIdx.x; n < N; n += 256)
            a = fma(yp[n], yp[n] / ep[n], a);
        a = sp_block_sum(a, sh);
        if (threadIdx.x == 0)
            out[1 + p] = a;
    }
}

// Zw[n, i] = w_n Z[n, i] (the composed Gram path's weighted operand; same layout)
__global__ __launch_bounds__(256) void k_sp_scale(const double* __restrict__ Z, int64_t sn, int64_t si, int64_t nc, int64_t M,
                                                  const double* __restrict__ w, double* __restrict__ Zw, int kmaj)
{
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    const int64_t n = kmaj ? a : b, i = kmaj ? b : a; // the contiguous index along the threads
    if (n < nc && i < M)
        Zw[n * sn + i * si] = w[n] * Z[n * sn + i * si];
}

// ---- the weighted Gram -------------------------------------------------------------------------------------------------
// mode 0: the partial tile -> Out + slot pstride (a partial matrix, ldo); 1: A's tile = the product; 2: A's tile += the product.
// Out has round_up(M, 64) rows and columns behind it: whole tiles are stored (rows / columns beyond M are zero).
template <bool KMAJ>
__global__ __launch_bounds__(256, 4) void k_sp_gram(const double* __restrict__ Z, int64_t sn, int64_t si, const double* __restrict__ w,
                                                    int64_t n0, int64_t M, const int64_t* __restrict__ plan, int64_t slot0,
                                                    double* __restrict__ Out, int64_t ldo, int64_t pstride, int mode)
{
    __shared__ double As[GT * GLD]; // [row of the tile][k], weighted
    __shared__ double Bs[GT * GLD]; // [column of the tile][k]
    const int64_t* pr = plan + (int64_t)blockIdx.x * 5;
    const int64_t ti = pr[0], tj = pr[1], k0 = pr[2] - n0, k1 = pr[3] - n0, slot = pr[4] - slot0;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    // staging: 8 elements of either operand per thread and step, the contiguous index along the threads: element q of a thread is
    // (row er + 8 q, column ek) of the 64 x 32 step when k is contiguous, (row er, column ek + 4 q) otherwise — one base address
    // per operand and a uniform stride
    const int er = KMAJ ? t >> 5 : t & 63, ek = KMAJ ? t & 31 : t >> 6;
    const int64_t qs = KMAJ ? 8 * si : 4 * sn;
    const double* pa = Z + (ti * GT + er) * si + (k0 + ek) * sn;
    const double* pb = Z + (tj * GT + er) * si + (k0 + ek) * sn;
    const double* pw = w + k0 + ek;
    const int64_t ra_rows = M - ti * GT - er, rb_rows = M - tj * GT - er; // > 0 (> 8 q): the row exists
    double ra[8], rb[8];
    auto fetch = [&](int64_t k) { // (k: the step's first column, k0 <= k < k1)
        const int64_t left = k1 - k - ek; // > 0 (> 4 q): the column exists
        if (KMAJ) {
            const double wn = left > 0 ? *pw : 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                ra[q] = left > 0 && ra_rows > 8 * q ? wn * pa[q * qs] : 0.0;
                rb[q] = left > 0 && rb_rows > 8 * q ? pb[q * qs] : 0.0;
            }
        }
        else {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                ra[q] = left > 4 * q && ra_rows > 0 ? pw[4 * q] * pa[q * qs] : 0.0;
                rb[q] = left > 4 * q && rb_rows > 0 ? pb[q * qs] : 0.0;
            }
        }
        pa += GKC * sn;
        pb += GKC * sn;
        pw += GKC;
    };
    d4_t acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
        acc[c] = d4_t{0.0, 0.0, 0.0, 0.0};
    // the instruction's operands (v_mfma_f64_16x16x4_f64: one f64 per lane, first operand P[x = lane & 15][k = lane >> 4], second
    // Q[k = lane >> 4][y = lane & 15], result D[x = (lane >> 4) + 4 reg][y = lane & 15]).  x = the tile's COLUMN (this wave's 16),
    // y = the tile's ROW: a result register's 16 lanes are 16 consecutive rows of one column — contiguous in the column-major tile.
    const int fr = lane & 15, fk = lane >> 4;
    const double* bp = Bs + (16 * wv + fr) * GLD + fk;
    const double* ap = As + fr * GLD + fk;
    fetch(k0);
    for (int64_t k = k0; k < k1; k += GKC) {
        __syncthreads(); // (the previous step's reads are done)
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int o = KMAJ ? (er + 8 * q) * GLD + ek : er * GLD + ek + 4 * q;
            As[o] = ra[q];
            Bs[o] = rb[q];
        }
        __syncthreads();
        if (k + GKC < k1)
            fetch(k + GKC);
#pragma unroll
        for (int kk = 0; kk < GKC; kk += 4) {
            const double b = bp[kk];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                acc[c] = mfma_f64(b, ap[16 * c * GLD + kk], acc[c]);
        }
    }
    double* o = Out + (mode == 0 ? slot * pstride : 0);
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t i = ti * GT + 16 * c + fr, j = tj * GT + 16 * wv + fk + 4 * r;
            double* d = o + i + j * ldo;
            *d = mode == 2 ? *d + acc[c][r] : acc[c][r];
        }
}

// A's lower tiles (=, first) or (+=) the sum of the nsl partial matrices in ascending slot
__global__ __launch_bounds__(256) void k_sp_fold(const double* __restrict__ Part, int64_t ldp, int64_t pstride, int nsl, int first,
                                                 double* __restrict__ A, int64_t lda)
{
    const int t = (int)blockIdx.x;
    int ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((ti + 1) * (ti + 2) / 2 <= t)
        ++ti;
    while (ti * (ti + 1) / 2 > t)
        --ti;
    const int tj = t - ti * (ti + 1) / 2;
    const int r = threadIdx.x & 63;
    for (int cc = threadIdx.x >> 6; cc < GT; cc += 4) {
        const int64_t i = (int64_t)ti * GT + r, j = (int64_t)tj * GT + cc;
        double s = Part[i + j * ldp];
        for (int q = 1; q < nsl; ++q)
            s += Part[(int64_t)q * pstride + i + j * ldp];
        double* d = A + i + j * lda;
        *d = first ? s : *d + s;
    }
}

__global__ void k_sp_diag_add(double* __restrict__ A, int64_t lda, int64_t M, double v)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < M)
        A[i + i * lda] += v;
}

// s2[t] = v1[t] - sig v2[t]   (v1 = c - |lst|^2, v2 = -|lmst|^2: spgp.hpp:608 without the "+ sig")
__global__ void k_sp_s2(const double* __restrict__ v1, const double* __restrict__ v2, double sig, int64_t T, double* __restrict__ s2)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < T)
        s2[i] = v1[i] - sig * v2[i];
}

void launch_sp_ep(hipStream_t s, const double* Z, int64_t sn, int64_t si, int64_t nc, int64_t M, double c, double sig, double* ep, double* w)
{
    if (nc > 0)
        GPE_LAUNCH(k_sp_ep, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, s, Z, sn, si, nc, M, c, sig, ep, w);
}
void launch_sp_r(hipStream_t s, const double* Z, int64_t sn, int64_t si, int64_t nc, int64_t M, const double* w, const double* y, int64_t ldy,
                 int P, double* R, int64_t ldr)
{
    if (nc > 0 && M > 0 && P > 0)
        GPE_LAUNCH(k_sp_r, dim3((unsigned)M, (unsigned)P), dim3(256), 0, s, Z, sn, si, nc, w, y, ldy, R, ldr);
}
void launch_sp_sums(hipStream_t s, const double* ep, int64_t N, const double* y, int64_t ldy, int P, double* out)
{
    GPE_LAUNCH(k_sp_sums, dim3(1), dim3(256), 0, s, ep, N, y, ldy, P, out);
}
void launch_sp_scale(hipStream_t s, const double* Z, int64_t sn, int64_t si, int64_t nc, int64_t M, const double* w, double* Zw)
{
    if (nc <= 0 || M <= 0)
        return;
    const int kmaj = sn == 1;
    const int64_t a = kmaj ? nc : M, b = kmaj ? M : nc;
    GPE_LAUNCH(k_sp_scale, dim3((unsigned)((a + 255) / 256), (unsigned)b), dim3(256), 0, s, Z, sn, si, nc, M, w, Zw, kmaj);
}
void launch_sp_gram(hipStream_t s, const double* Z, int64_t sn, int64_t si, const double* w, int64_t n0, int64_t M, const int64_t* plan,
                    int64_t rows, int64_t slot0, double* Out, int64_t ldo, int64_t pstride, int mode)
{
    if (rows <= 0)
        return;
    if (sn == 1)
        GPE_LAUNCH((k_sp_gram<true>), dim3((unsigned)rows), dim3(256), 0, s, Z, sn, si, w, n0, M, plan, slot0, Out, ldo, pstride, mode);
    else
        GPE_LAUNCH((k_sp_gram<false>), dim3((unsigned)rows), dim3(256), 0, s, Z, sn, si, w, n0, M, plan, slot0, Out, ldo, pstride, mode);
}
void launch_sp_fold(hipStream_t s, const double* Part, int64_t ldp, int64_t pstride, int nsl, int first, int64_t M, double* A, int64_t lda)
{
    const int64_t nt = (M + GT - 1) / GT;
    GPE_LAUNCH(k_sp_fold, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, s, Part, ldp, pstride, nsl, first, A, lda);
}
void launch_sp_diag_add(hipStream_t s, double* A, int64_t lda, int64_t M, double v)
{
    GPE_LAUNCH(k_sp_diag_add, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, A, lda, M, v);
}
void launch_sp_s2(hipStream_t s, const double* v1, const double* v2, double sig, int64_t T, double* s2)
{
    if (T > 0)
        GPE_LAUNCH(k_sp_s2, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, v1, v2, sig, T, s2);
}
