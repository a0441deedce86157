// append.hip — the device tail of a blocked append (include/gpe_append.h): q <= AP_CHUNK new samples V join a factor of order n.
//
//   Zt[a + k ldq] = (L^-1 k(X, v_a))_k            the transposed layout of query.hpp, left by chunk_solve
//   S  = k(V, V) + diag_add I - Zt Zt^T           gp.hpp:583-597 for a block; C = chol(S), lower
//   L[n + a, k] = Zt[a, k]  (k < n),   L[n + a, n + b] = C[a, b]
//
// Three launches, whatever q is:
//   k_append_syrk    the k range (length n) cut into slices, one workgroup each: the slice's share of Zt Zt^T into partial
//                    matrix `slice`, and — it has the slice of Zt in LDS anyway — the slice's columns of the q new rows of L
//                    (both sides contiguous in a)
//   k_append_fold    S = k(v_a, v_b) (+ diag_add on the diagonal) - the partials in ascending slice: a fixed order, no
//                    floating-point atomics, bitwise reproducible whatever CUs were free
//   k_append_factor  one workgroup: S in LDS (128 x 128 doubles = 128 KiB of gfx950's 160), right-looking Cholesky, C stored at
//                    (n, n) of the factor — n is in general no multiple of 64 — and the pivot word
// The diagonal-block inverses of every 64-block that gained rows are refreshed by the caller (launch_diag_inv).
#include <algorithm>

#include "dev.h"

#define AP_CHUNK 128 // rows the tail factorises at once (gpe_append_max_chunk)
#define AP_KT 16     // k step of the partial product

int append_max_chunk() { return AP_CHUNK; }

// slices of the k range: 256 columns each, from 65 536 samples on as many more as keep the slices at 256
void append_slices(int64_t n, int64_t* kslice, int* nsl)
{
    int64_t ks = 256;
    if ((n + ks - 1) / ks > 256)
        ks = ((n + 255) / 256 + AP_KT - 1) / AP_KT * AP_KT;
    *kslice = ks;
    *nsl = (int)std::max<int64_t>(1, (n + ks - 1) / ks);
}
// An upper bound of the slice count of EVERY order <= n: up to 65 536 samples the count is ceil(n / 256), which grows with n;
// beyond, the slices widen in steps of 16 columns and the count moves up and down below 256 (65 536: 256 slices, 65 537: 241).
// A call whose chunks see orders n0 .. nfin reserves for this bound of nfin and lays the partial matrices out by it.
int append_slices_cap(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(256, (n + 255) / 256)); }
size_t append_scratch_doubles(int64_t n) { return (size_t)(append_slices_cap(n) + 1) * AP_CHUNK * AP_CHUNK; }

// RT x RT accumulators per thread, thread (tx, ty) of 16 x 16 owns rows tx + 16 i and columns ty + 16 j: the LDS reads of a wave
// are 16 consecutive doubles (a) and 4 broadcast addresses (b) — no bank conflicts.  RT = 4 covers q <= 64, RT = 8 q <= 128.
template <int RT>
__global__ __launch_bounds__(256) void k_append_syrk(const double* __restrict__ Zt, int64_t ldq, int q, int64_t n, int64_t kslice,
                                                     double* __restrict__ Part, double* __restrict__ Lrows, int64_t ld)
{
    constexpr int W = 16 * RT; // rows held in LDS
    __shared__ double zs[AP_KT][W];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double acc[RT][RT];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < RT; ++j)
            acc[i][j] = 0.0;
    const int64_t k0 = (int64_t)blockIdx.x * kslice;
    const int64_t k1 = k0 + kslice < n ? k0 + kslice : n;
    for (int64_t kb = k0; kb < k1; kb += AP_KT) {
        __syncthreads();
        for (int e = threadIdx.x; e < AP_KT * W; e += 256) {
            const int kk = e / W, a = e % W;
            const int64_t k = kb + kk;
            double v = 0.0;
            if (a < q && k < k1) {
                v = Zt[a + k * ldq];
                Lrows[a + k * ld] = v; // L[n + a, k]
            }
            zs[kk][a] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < AP_KT; ++kk) {
            double av[RT], bv[RT];
#pragma unroll
            for (int i = 0; i < RT; ++i) {
                av[i] = zs[kk][tx + 16 * i];
                bv[i] = zs[kk][ty + 16 * i];
            }
#pragma unroll
            for (int i = 0; i < RT; ++i)
#pragma unroll
                for (int j = 0; j < RT; ++j)
                    acc[i][j] = fma(av[i], bv[j], acc[i][j]);
        }
    }
    double* P = Part + (int64_t)blockIdx.x * (AP_CHUNK * AP_CHUNK);
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < RT; ++j) {
            const int a = tx + 16 * i, b = ty + 16 * j;
            if (a < q && b <= a)
                P[a + b * AP_CHUNK] = acc[i][j];
        }
}

// S[a, b] (lower, ld AP_CHUNK) = k(v_a, v_b) + diag_add [a == b] - sum_s Part_s[a, b]
__global__ __launch_bounds__(256) void k_append_fold(const double* __restrict__ Part, int nsl, const double* __restrict__ Qt, int64_t ldq,
                                                     int q, KParams kp, double* __restrict__ S)
{
    const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const int a = e % AP_CHUNK, b = e / AP_CHUNK;
    if (a >= q || b > a)
        return;
    double z = 0.0;
    for (int d = 0; d < kp.D; ++d) {
        // the difference is scaled, as k_build does (kbuild.hip)
        const double t = (Qt[(int64_t)d * ldq + a] - Qt[(int64_t)d * ldq + b]) * kp.inv_ell[d];
        z = fma(t, t, z);
    }
    double acc = 0.0;
    for (int s = 0; s < nsl; ++s) // ascending k: the fixed order of the reduction
        acc += Part[(int64_t)s * (AP_CHUNK * AP_CHUNK) + a + b * AP_CHUNK];
    double v = kfun(kp.kind, z, kp.sf2); // no noise off the diagonal, even between coincident points (kernel.hpp:81-84)
    if (a == b)
        v += kp.diag_add;
    S[a + b * AP_CHUNK] = v - acc;
}

// C = chol(S) in LDS, column-major (rows contiguous: a wave's accesses of one column are consecutive doubles, the pivot column is
// read through a copy that every lane broadcasts from).  Two barriers per column.  C goes to Cout[a + b ldc], b <= a; the first
// non-positive (or NaN) pivot j is reported as goff + j + 1 if the word is still 0, the square root then carries NaN on.
__global__ __launch_bounds__(256) void k_append_factor(const double* __restrict__ S, int q, double* __restrict__ Cout, int64_t ldc,
                                                       int* __restrict__ info, int64_t goff)
{
    __shared__ double Ss[AP_CHUNK * AP_CHUNK];
    __shared__ double col[AP_CHUNK];
    __shared__ double dg[AP_CHUNK];
    const int tid = threadIdx.x;
    for (int e = tid; e < AP_CHUNK * q; e += 256) {
        const int a = e % AP_CHUNK, b = e / AP_CHUNK;
        if (a < q && b <= a)
            Ss[a + b * AP_CHUNK] = S[a + b * AP_CHUNK];
    }
    const int i = tid & (AP_CHUNK - 1), half = tid >> 7;
    bool flagged = false;
    for (int j = 0; j < q; ++j) {
        __syncthreads(); // the update of step j - 1 is complete
        const double d = Ss[j + j * AP_CHUNK];
        const double r = sqrt(d);
        if (tid == 0) {
            if (!(d > 0.0) && !flagged) {
                flagged = true;
                if (*info == 0)
                    *info = (int)(goff + j + 1);
            }
            dg[j] = r; // (the diagonal keeps d in Ss: nobody waits for this store)
        }
        if (half == 0 && i > j && i < q) {
            const double v = Ss[i + j * AP_CHUNK] / r;
            Ss[i + j * AP_CHUNK] = v;
            col[i] = v;
        }
        __syncthreads();
        if (i > j && i < q) {
            const double li = col[i];
            for (int c = j + 1 + half; c <= i; c += 2)
                Ss[i + c * AP_CHUNK] = fma(-li, col[c], Ss[i + c * AP_CHUNK]);
        }
    }
    __syncthreads();
    for (int e = tid; e < AP_CHUNK * q; e += 256) {
        const int a = e % AP_CHUNK, b = e / AP_CHUNK;
        if (a < q && b <= a)
            Cout[a + (int64_t)b * ldc] = a == b ? dg[a] : Ss[a + b * AP_CHUNK];
    }
}

// scratch: slices_cap partial matrices, then S (append_scratch_doubles of the largest order the call reaches).  Zt, Qt: the chunk's
// buffers of query.hpp (ldq).  Returns false, with nothing launched, for a chunk or a slice count the scratch was not sized for.
bool launch_append_tail(hipStream_t s, const double* Zt, const double* Qt, int64_t ldq, int q, int64_t n, const KParams& kp, double* A,
                        int64_t ld, int* info, double* scratch, int slices_cap)
{
    if (q <= 0 || q > AP_CHUNK)
        return false;
    int64_t kslice;
    int nsl;
    append_slices(n, &kslice, &nsl);
    if (nsl > slices_cap)
        return false;
    double* Part = scratch;
    double* S = scratch + (size_t)slices_cap * AP_CHUNK * AP_CHUNK;
    if (q <= 64)
        GPE_LAUNCH(k_append_syrk<4>, dim3((unsigned)nsl), dim3(256), 0, s, Zt, ldq, q, n, kslice, Part, A + n, ld);
    else
        GPE_LAUNCH(k_append_syrk<8>, dim3((unsigned)nsl), dim3(256), 0, s, Zt, ldq, q, n, kslice, Part, A + n, ld);
    GPE_LAUNCH(k_append_fold, dim3((unsigned)((AP_CHUNK * q + 255) / 256)), dim3(256), 0, s, Part, nsl, Qt, ldq, q, kp, S);
    GPE_LAUNCH(k_append_factor, dim3(1), dim3(256), 0, s, S, q, A + n + n * ld, ld, info, n);
    return true;
}
