// remove.hip — the device side of gpe_remove_samples (include/gpe_remove.h): a <= GPE_RM_CAP samples leave a factor of order n.
//
// Sweep the columns c = i0 .. n - 1 of the old factor.  A removed column's part below the diagonal becomes update vector u_k
// (row and column c disappear); a kept column absorbs the live vectors: with d = L[c, c] and u = (u_0[c] .. u_{a-1}[c]),
//   d' = sqrt(d^2 + |u|^2),   w = (d - d', u) = (w0, u),   w0 = -|u|^2 / (d + d')   (no cancellation),   beta = -1 / (d' w0)
// and every row r > c takes (L[r, c], u[r]) <- (L[r, c], u[r]) (I - beta w w^T): a reflector that maps (d, u) to (d', 0), so the
// diagonal stays positive, u_k[c] is zero afterwards and L L^T + U U^T is kept — the per-column form of the Givens sweep, with
// one square root per column instead of one per column and vector, and 2 a + 2 fused multiply-adds per element.  Vectors not yet
// born are zero and ride along.  No pivot can fail (d' >= d); NaNs propagate.
//
// The bound is HBM: every element of the trailing part is read once and written once, to its COMPACTED place
// (r - removed_before(r), c - removed_before(c)) in a second matrix — compaction moves elements across workgroups, in place it
// races.  Per 256-column panel of the old factor two launches:
//   k_rm_rot    one workgroup, thread t owns row c0 + t of the panel's triangle and its a values of U in registers.  Columns are
//               sequential: the diagonal thread forms the reflector, one barrier hands it over through LDS, the rows below apply
//               it.  The triangle passes through LDS 64 columns at a time (a thread's own row of them), so that nothing on the
//               column-to-column chain waits for HBM; behind a slab its finished rows go to their destination and its reflectors
//               to a table in global memory.
//   k_rm_apply  every row below the panel, one lane per row, a wave per workgroup: 64 consecutive rows, so a column is one
//               contiguous 512-byte segment on both sides.  U in registers (a = 32: 64 VGPRs), the table staged through LDS 64
//               columns at a time, the factor's values loaded 8 to 32 columns ahead (a panel has one wave per 64 rows: the
//               loads in flight come from the depth).  U goes back to an n x a buffer between panels.
// No workgroup waits for another inside a launch.  Same input, same launches, same order: bitwise reproducible.
#include <algorithm>

#include "dev.h"

int remove_max_vectors() { return GPE_RM_CAP; }
size_t remove_u_ld(int64_t n) { return (size_t)((n + 63) / 64 * 64); }
size_t remove_coef_doubles() { return (size_t)GPE_RM_PANEL * (GPE_RM_CAP + 2); }

// removed indices below x, and the vector born at x (-1: x stays); R is a kernel argument: uniform, scalar registers
__device__ __forceinline__ int rm_before(const RmList& R, int x)
{
    int b = 0;
#pragma unroll
    for (int k = 0; k < GPE_RM_CAP; ++k)
        b += (k < R.a && R.idx[k] < x) ? 1 : 0;
    return b;
}
__device__ __forceinline__ int rm_slot(const RmList& R, int x)
{
    int s = -1;
#pragma unroll
    for (int k = 0; k < GPE_RM_CAP; ++k)
        s = (k < R.a && R.idx[k] == x) ? k : s;
    return s;
}

__global__ __launch_bounds__(256) void k_rm_xt(double* __restrict__ Xt, int64_t ld, const int* __restrict__ keep, int64_t n_new, int64_t n_old)
{
    double* X = Xt + (int64_t)blockIdx.x * ld;
    // a chunk reads at keep[j] >= j and writes at j: what earlier chunks wrote lies below everything later chunks read
    for (int64_t base = 0; base < n_old; base += 256) {
        const int64_t j = base + threadIdx.x;
        const double v = j < n_new ? X[keep[j]] : 0.0;
        __syncthreads();
        if (j < n_old)
            X[j] = v;
    }
}

__global__ __launch_bounds__(256) void k_rm_head(const double* __restrict__ src, double* __restrict__ dst, int64_t ld, int n, int ch, RmList R)
{
    const int r = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const int cb0 = (int)blockIdx.y * 32;
    if (r >= n || r < cb0 || rm_slot(R, r) >= 0)
        return;
    const int rn = r - rm_before(R, r);
    const int ce = min(min(cb0 + 32, ch), r + 1);
    for (int c = cb0; c < ce; ++c)
        dst[rn + (int64_t)c * ld] = src[r + (int64_t)c * ld];
}

// the reflector of a kept column from its diagonal d and the vectors' values u there: cf[0] = w0, cf[1] = beta, cf[2 + k] = u[k]
template <int A> __device__ __forceinline__ double rm_reflector(double d, const double (&u)[A], double* cf)
{
    double sp[4] = {0.0, 0.0, 0.0, 0.0}; // four partial sums: the diagonal thread's chain is the launch's critical path
#pragma unroll
    for (int k = 0; k < A; ++k)
        sp[k & 3] = fma(u[k], u[k], sp[k & 3]);
    const double sg = (sp[0] + sp[1]) + (sp[2] + sp[3]);
    double w0 = 0.0, beta = 0.0, dn = d;
    if (!(sg < 1e-290)) { // (below: the identity to rounding; a NaN goes on)
        dn = sqrt(fma(d, d, sg));
        w0 = -sg / (d + dn);
        beta = (d + dn) / (dn * sg); // = -1 / (dn w0)
    }
#pragma unroll
    for (int k = 0; k < A; ++k)
        cf[2 + k] = u[k];
    cf[0] = w0;
    cf[1] = beta;
    return dn;
}

// the pass's indices in LDS, closed by a sentinel: the sweep keeps the position of the next removed column and reads one entry
// when it gets there (a dynamic index into the kernel argument itself would move the list to scratch memory)
__device__ __forceinline__ void rm_stage_list(const RmList& R, int* ridx)
{
    if (threadIdx.x <= GPE_RM_CAP) {
        int v = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < GPE_RM_CAP; ++k)
            v = ((int)threadIdx.x == k && k < R.a) ? R.idx[k] : v;
        ridx[threadIdx.x] = v;
    }
}

#define RM_SLAB 64 // columns of the triangle a thread keeps in LDS at a time (its own row of them: nobody else reads it)

template <int A>
__global__ __launch_bounds__(256) void k_rm_rot(const double* __restrict__ src, double* __restrict__ dst, int64_t ld, int c0, int w, RmList R,
                                                int first, const double* __restrict__ U, int64_t ldu, double* __restrict__ coef)
{
    // between the load of a slab and its write-back the sweep touches LDS only: no wait for HBM on the column-to-column chain
    __shared__ double slab[RM_SLAB * 256];
    __shared__ double ctab[RM_SLAB * (A + 2)];
    __shared__ int ridx[GPE_RM_CAP + 1];
    const int t = (int)threadIdx.x, r = c0 + t;
    const bool inr = t < w;
    rm_stage_list(R, ridx);
    // every load below is unconditional, from a clamped row: a load under a per-lane condition is a branch and a full wait each
    const int rr = min(r, c0 + w - 1);
    double u[A];
#pragma unroll
    for (int k = 0; k < A; ++k)
        u[k] = 0.0;
    if (!first) {
#pragma unroll
        for (int k = 0; k < A; ++k)
            u[k] = U[rr + (int64_t)k * ldu];
    }
    const int rn = r - rm_before(R, r);
    const bool rowkept = inr && rm_slot(R, r) < 0;
    int nk = rm_before(R, c0); // the next removed column is R.idx[nk]: as many are in front of the current one
    __syncthreads();
    int nextc = ridx[nk];
    for (int s0 = 0; s0 < w; s0 += RM_SLAB) {
        const int ws = min(RM_SLAB, w - s0);
#pragma unroll 8
        for (int jj = 0; jj < ws; ++jj) {
            const int c = c0 + s0 + jj;
            slab[jj * 256 + t] = src[rr + (int64_t)c * ld]; // (above the diagonal: whatever lies there, never used below)
        }
        const int nk0 = nk;
        for (int jj = 0; jj < ws; ++jj) {
            const int j = s0 + jj, c = c0 + j;
            double l = slab[jj * 256 + t];
            if (c == nextc) { // the column becomes vector nk; nothing is stored
#pragma unroll
                for (int k = 0; k < A; ++k)
                    u[k] = (k == nk && r > c) ? l : u[k];
                nextc = ridx[++nk];
                continue;
            }
            double* cf = ctab + jj * (A + 2);
            if (t == j)
                l = rm_reflector<A>(l, u, cf);
            __syncthreads();
            if (inr && r > c) {
                const double w0 = cf[0];
                double sq[4] = {w0 * l, 0.0, 0.0, 0.0};
#pragma unroll
                for (int k = 0; k < A; ++k)
                    sq[(k + 1) & 3] = fma(cf[2 + k], u[k], sq[(k + 1) & 3]);
                const double sc = ((sq[0] + sq[1]) + (sq[2] + sq[3])) * cf[1];
                l = fma(-sc, w0, l);
#pragma unroll
                for (int k = 0; k < A; ++k)
                    u[k] = fma(-sc, cf[2 + k], u[k]);
            }
            else if (t == j) {
#pragma unroll
                for (int k = 0; k < A; ++k)
                    u[k] = 0.0;
            }
            slab[jj * 256 + t] = l;
        }
        // the slab's finished rows to their destination, its reflectors to the table
        int fk = nk0, fnext = ridx[fk];
        for (int jj = 0; jj < ws; ++jj) {
            const int c = c0 + s0 + jj;
            if (c == fnext) {
                fnext = ridx[++fk];
                continue;
            }
            if (rowkept && r >= c)
                dst[rn + (int64_t)(c - fk) * ld] = slab[jj * 256 + t];
        }
        for (int e = t; e < ws * (A + 2); e += 256)
            coef[(int64_t)s0 * (A + 2) + e] = ctab[e];
        __syncthreads(); // (the next slab's first reflector overwrites the table)
    }
}

template <int A>
__global__ __launch_bounds__(64) void k_rm_apply(const double* __restrict__ src, double* __restrict__ dst, int64_t ld, int n, int c0, int w,
                                                 RmList R, int first, double* __restrict__ U, int64_t ldu, const double* __restrict__ coef)
{
    constexpr int G = A <= 8 ? 32 : (A <= 16 ? 16 : 8); // columns loaded ahead: one wave per 64 rows, so the loads in flight come from here
    __shared__ double cs[64 * (A + 2)];
    __shared__ int ridx[GPE_RM_CAP + 1];
    const int t = (int)threadIdx.x, r = c0 + w + (int)blockIdx.x * 64 + t;
    const bool inr = r < n;
    rm_stage_list(R, ridx);
    // (unconditional loads from a clamped row and column, as in k_rm_rot)
    const int rr = min(r, n - 1);
    double u[A];
#pragma unroll
    for (int k = 0; k < A; ++k)
        u[k] = 0.0;
    if (!first) {
#pragma unroll
        for (int k = 0; k < A; ++k)
            u[k] = U[rr + (int64_t)k * ldu];
    }
    const int rn = r - rm_before(R, r);
    const bool rowkept = inr && rm_slot(R, r) < 0;
    int nk = rm_before(R, c0);
    __syncthreads();
    int nextc = ridx[nk];
    for (int j0 = 0; j0 < w; j0 += 64) {
        const int wc = min(64, w - j0);
        __syncthreads();
        for (int e = t; e < wc * (A + 2); e += 64)
            cs[e] = coef[(int64_t)j0 * (A + 2) + e];
        __syncthreads();
        for (int j1 = 0; j1 < wc; j1 += G) {
            double lg[G];
#pragma unroll
            for (int q = 0; q < G; ++q)
                lg[q] = src[rr + (int64_t)min(c0 + j0 + j1 + q, c0 + w - 1) * ld];
#pragma unroll
            for (int q = 0; q < G; ++q) {
                const int jj = j1 + q, c = c0 + j0 + jj;
                if (jj >= wc)
                    break;
                double l = lg[q];
                if (c == nextc) {
#pragma unroll
                    for (int k = 0; k < A; ++k)
                        u[k] = (k == nk) ? l : u[k];
                    nextc = ridx[++nk];
                    continue;
                }
                const double* cf = cs + jj * (A + 2);
                const double w0 = cf[0];
                double sq[4] = {w0 * l, 0.0, 0.0, 0.0};
#pragma unroll
                for (int k = 0; k < A; ++k)
                    sq[(k + 1) & 3] = fma(cf[2 + k], u[k], sq[(k + 1) & 3]);
                const double sc = ((sq[0] + sq[1]) + (sq[2] + sq[3])) * cf[1];
                l = fma(-sc, w0, l);
#pragma unroll
                for (int k = 0; k < A; ++k)
                    u[k] = fma(-sc, cf[2 + k], u[k]);
                if (rowkept)
                    dst[rn + (int64_t)(c - nk) * ld] = l;
            }
        }
    }
    if (inr) {
#pragma unroll
        for (int k = 0; k < A; ++k)
            U[r + (int64_t)k * ldu] = u[k];
    }
}

void launch_rm_xt(hipStream_t s, double* Xt, int64_t ld, int rows, const int* keep, int64_t n_new, int64_t n_old)
{
    if (rows > 0 && n_old > 0)
        GPE_LAUNCH(k_rm_xt, dim3((unsigned)rows), dim3(256), 0, s, Xt, ld, keep, n_new, n_old);
}

void launch_rm_head(hipStream_t s, const double* src, double* dst, int64_t ld, int64_t n, int64_t ch, const RmList& R)
{
    if (ch > 0)
        GPE_LAUNCH(k_rm_head, dim3((unsigned)((n + 255) / 256), (unsigned)((ch + 31) / 32)), dim3(256), 0, s, src, dst, ld, (int)n, (int)ch, R);
}

template <int A>
static int rm_panel(hipStream_t s, const double* src, double* dst, int64_t ld, int64_t n, int64_t c0, const RmList& R, bool first, double* U,
                    int64_t ldu, double* coef)
{
    const int w = (int)std::min<int64_t>(GPE_RM_PANEL, n - c0);
    GPE_LAUNCH(k_rm_rot<A>, dim3(1), dim3(256), 0, s, src, dst, ld, (int)c0, w, R, first ? 1 : 0, (const double*)U, ldu, coef);
    const int64_t below = n - (c0 + w);
    if (below <= 0)
        return 1;
    GPE_LAUNCH(k_rm_apply<A>, dim3((unsigned)((below + 63) / 64)), dim3(64), 0, s, src, dst, ld, (int)n, (int)c0, w, R, first ? 1 : 0, U, ldu,
               (const double*)coef);
    return 2;
}

int launch_rm_panel(hipStream_t s, const double* src, double* dst, int64_t ld, int64_t n, int64_t c0, const RmList& R, bool first, double* U,
                    int64_t ldu, double* coef)
{
    // the vector count rounded up to an instantiation: the surplus vectors are never born and stay zero
    if (R.a <= 1)
        return rm_panel<1>(s, src, dst, ld, n, c0, R, first, U, ldu, coef);
    if (R.a <= 4)
        return rm_panel<4>(s, src, dst, ld, n, c0, R, first, U, ldu, coef);
    if (R.a <= 8)
        return rm_panel<8>(s, src, dst, ld, n, c0, R, first, U, ldu, coef);
    if (R.a <= 16)
        return rm_panel<16>(s, src, dst, ld, n, c0, R, first, U, ldu, coef);
    return rm_panel<GPE_RM_CAP>(s, src, dst, ld, n, c0, R, first, U, ldu, coef);
}
