// select.hip — greedy batch selection with hallucinated observations (include/gpe_batch_select.h): the per-round kernels.
//
//   c[m]   = k(v_m, v_j) - sum_i Zt[m, i] Zt[j, i] - sum_{s<t} W[m, s] W[j, s]       j = this round's pick, read from device memory
//   W[m,t] = c[m] / sqrt(c[j] + obs_noise),   var[m] -= W[m,t]^2,   then the scores of the next round and their arg-max
//
// One round = four launches, ordered by kernel boundaries alone (no workgroup waits for another, no counters, no atomics):
//   k_sel_gather   row j of Zt (strided by ldz) and row j of W into contiguous vectors, once — not in every workgroup
//   k_sel_colprod  the hot one, HBM-read bound: Zt z_j with the k range split over workgroups (sel_plan), one partial vector per
//                  (m-tile, k-chunk); lanes take consecutive m with 16-byte loads
//   k_sel_fold     per m: the partials in ascending slot, the kernel value, the rank-1 history, the pivot (recomputed by every
//                  workgroup for itself), W[:, t], var, the next score; one (value, lowest index) pair per workgroup
//   k_sel_pick     one workgroup: the pairs -> j_{t+1}, idx / score of that round, the failure round
// All q rounds are enqueued at once; after a failed pivot the remaining launches return at their first instruction (SelState::fail).
#include <algorithm>
#include <cfloat>

#include "dev.h"

namespace {
constexpr int SEL_TM = 256;    // m per workgroup of the column product: 128 lanes x 2 doubles, two k phases
constexpr int SEL_KSTEP = 16;  // chunk bounds are multiples of it
constexpr int SEL_KMIN = 32;   // no chunk shorter than this
constexpr int SEL_NCH_MAX = 512;
constexpr int SEL_FT = 64;      // candidates per workgroup of the fold (select_fold_groups: the host sizes `pairs` by it)
constexpr int SEL_UNROLL = 8;  // rows in flight per thread: 8 x 16 B x 256 threads = 32 KiB of loads per workgroup
} // namespace

// chunks the k range of every m-tile is cut into: enough workgroups for four per CU at any M, no chunk below SEL_KMIN
int select_chunks(int64_t M, int64_t N, int cus)
{
    const int64_t nmt = (M + SEL_TM - 1) / SEL_TM;
    const int64_t units = (N + SEL_KSTEP - 1) / SEL_KSTEP;
    int64_t nch = (4 * (int64_t)cus + nmt - 1) / nmt;
    nch = std::min<int64_t>(nch, std::max<int64_t>(1, units / (SEL_KMIN / SEL_KSTEP)));
    return (int)std::max<int64_t>(1, std::min<int64_t>(nch, SEL_NCH_MAX));
}

int select_fold_groups(int64_t M) { return (int)((M + SEL_FT - 1) / SEL_FT); }

// rows of 5: { m0, m1 (<= M), k0, k1 (<= N), partial slot }: one workgroup each, in launch order (chunk-major: the workgroups in
// flight together read the same rows of Zt and the same piece of z_j).  Returns the number of rows.
int select_plan(int64_t M, int64_t N, int cus, int64_t* out, int64_t cap_rows)
{
    if (M <= 0 || N <= 0 || cus <= 0)
        return -1;
    const int64_t nmt = (M + SEL_TM - 1) / SEL_TM;
    const int64_t units = (N + SEL_KSTEP - 1) / SEL_KSTEP;
    const int nch = select_chunks(M, N, cus);
    const int64_t base = units / nch, rem = units % nch;
    int64_t row = 0, u0 = 0;
    for (int c = 0; c < nch; ++c) {
        const int64_t u = base + (c < rem ? 1 : 0);
        const int64_t k0 = u0 * SEL_KSTEP, k1 = std::min<int64_t>((u0 + u) * SEL_KSTEP, N);
        for (int64_t i = 0; i < nmt; ++i, ++row) {
            if (!out || row >= cap_rows)
                continue;
            int64_t* o = out + row * 5;
            o[0] = i * SEL_TM;
            o[1] = std::min<int64_t>((i + 1) * SEL_TM, M);
            o[2] = k0;
            o[3] = k1;
            o[4] = c;
        }
        u0 += u;
    }
    return (int)row;
}

// Zt[m + i ldz] = Z[i + m ld]: the N x M layout of the small models into the layout of the rounds, once per call
__global__ __launch_bounds__(256) void k_sel_transpose(const double* __restrict__ Z, int64_t ld, int64_t N, int64_t M, double* __restrict__ Zt,
                                                       int64_t ldz)
{
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5; // 32 x 8
    const int64_t i0 = (int64_t)blockIdx.x * 32, m0 = (int64_t)blockIdx.y * 32;
    for (int r = ty; r < 32; r += 8) {
        const int64_t i = i0 + tx, m = m0 + r;
        tile[r][tx] = (i < N && m < M) ? Z[i + m * ld] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int64_t m = m0 + tx, i = i0 + r;
        if (m < M && i < N)
            Zt[m + i * ldz] = tile[tx][r];
    }
}

__global__ __launch_bounds__(256) void k_sel_gather(const SelState* __restrict__ st, const double* __restrict__ Zt, int64_t ldz, int64_t N,
                                                    const double* __restrict__ W, int64_t ldw, int t, double* __restrict__ zj,
                                                    double* __restrict__ wj)
{
    if (st->fail != 0)
        return;
    const int64_t j = st->j;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < N)
        zj[e] = Zt[j + e * ldz];
    else if (e - N < t)
        wj[e - N] = W[j + (e - N) * ldw];
}

// part[slot ldp + m] = sum_{k0 <= i < k1} Zt[m + i ldz] zj[i] for m0 <= m < m1.  thread = (pair of consecutive m, k phase of 2);
// the two phases are added in LDS, phase 0 first.  Zt's rows are 16-byte aligned (ldz even, m0 a multiple of SEL_TM) and ldz >= M
// rounded up to 2, so the second double of a pair is inside the row even where m + 1 == M (it is loaded and not stored).
__global__ __launch_bounds__(256) void k_sel_colprod(const SelState* __restrict__ st, const int64_t* __restrict__ plan,
                                                     const double* __restrict__ Zt, int64_t ldz, const double* __restrict__ zj,
                                                     double* __restrict__ part, int64_t ldp)
{
    if (st->fail != 0)
        return;
    __shared__ double2 red[128];
    const int64_t* row = plan + (int64_t)blockIdx.x * 5;
    const int64_t m0 = row[0], m1 = row[1], k0 = row[2], k1 = row[3], slot = row[4];
    const int lane = threadIdx.x & 127, ph = threadIdx.x >> 7;
    const int64_t m = m0 + 2 * lane;
    const bool live = m < m1;
    double a0 = 0.0, a1 = 0.0;
    if (live) {
        const double* zp = Zt + m;
        int64_t i = k0 + ph;
        for (; i + 2 * (SEL_UNROLL - 1) < k1; i += 2 * SEL_UNROLL) {
            double2 v[SEL_UNROLL];
            double z[SEL_UNROLL];
#pragma unroll
            for (int u = 0; u < SEL_UNROLL; ++u) {
                v[u] = *(const double2*)(zp + (i + 2 * u) * ldz);
                z[u] = zj[i + 2 * u];
            }
#pragma unroll
            for (int u = 0; u < SEL_UNROLL; ++u) {
                a0 = fma(v[u].x, z[u], a0);
                a1 = fma(v[u].y, z[u], a1);
            }
        }
        for (; i < k1; i += 2) {
            const double2 v = *(const double2*)(zp + i * ldz);
            const double z = zj[i];
            a0 = fma(v.x, z, a0);
            a1 = fma(v.y, z, a1);
        }
    }
    if (ph == 1)
        red[lane] = make_double2(a0, a1);
    __syncthreads();
    if (ph == 0 && live) {
        const double2 o = red[lane];
        double* p = part + slot * ldp + m;
        p[0] = a0 + o.x;
        if (m + 1 < m1)
            p[1] = a1 + o.y;
    }
}

// the score of one candidate (include/gpe_batch_select.h)
static __device__ __forceinline__ double sel_score(int rule, double mu, double var, double var_add, double param)
{
    const double s2 = (var <= DBL_EPSILON ? 0.0 : var) + var_add;
    if (rule == SEL_RULE_VAR)
        return s2;
    const double sigma = sqrt(s2);
    if (rule == SEL_RULE_UCB)
        return mu + param * sigma;
    if (sigma < 1e-10) // acqui/ei.hpp: _value
        return 0.0;
    const double X = mu - param, Z = X / sigma;
    const double phi = exp(-0.5 * Z * Z) / 2.50662827463100050242; // sqrt(2 pi)
    const double Phi = 0.5 * erfc(-Z * 0.70710678118654752440);
    return X * Phi + sigma * phi;
}

// the workgroup's largest value and the lowest index that holds it (-1: no thread has a candidate), left in sv[0] / si[0]; T threads
template <int T>
static __device__ __forceinline__ void sel_best(double* sv, long long* si, double bv, long long bi)
{
    sv[threadIdx.x] = bv;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int w = T / 2; w > 0; w >>= 1) {
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
}

// t >= 0: round t's column, then the scores of round t + 1;  t < 0: the scores of round 0 only.
// One workgroup (one wave) per SEL_FT candidates, thread = candidate: few candidates still spread over many compute units, and a
// thread's chain of nch partials is what bounds the launch (measured at (N, M) = (16 384, 1024), nch = 256: 126 us with 256
// candidates per workgroup, the pivot's chain walked by one thread and the loads issued one by one).
// c[m] = the kernel value less the partials in ascending slot — the fixed order of the reduction; the loads are unrolled so that
// 16 are in flight — less the rank-1 history.  The pivot c[j] is formed by every workgroup for itself, from the same numbers in
// the same order: j's partials are fetched by the lanes side by side into LDS and added from there, ascending.
// pairs[2 wg] = the largest score, pairs[2 wg + 1] = the bits of the lowest index that holds it (-1: none is eligible).
__global__ __launch_bounds__(SEL_FT) void k_sel_fold(SelState* __restrict__ st, const double* __restrict__ part, int64_t ldp, int nch,
                                                     const double* __restrict__ Qt, int64_t ldq, int64_t M, KParams kp,
                                                     double* __restrict__ W, int64_t ldw, const double* __restrict__ wj, int t,
                                                     double* __restrict__ var, const double* __restrict__ mu, int* __restrict__ picked,
                                                     int rule, double param, double var_add, double obs_noise, int distinct,
                                                     double* __restrict__ pairs)
{
    __shared__ double sv[SEL_FT];
    __shared__ long long si[SEL_FT];
    __shared__ double s_pj[SEL_NCH_MAX];
    if (st->fail != 0)
        return;
    const int64_t m = (int64_t)blockIdx.x * SEL_FT + threadIdx.x;
    const int64_t j = t >= 0 ? st->j : -1;
    if (t >= 0) {
        for (int c = threadIdx.x; c < nch; c += SEL_FT)
            s_pj[c] = part[(int64_t)c * ldp + j];
        __syncthreads();
        double accj = s_pj[0];
        for (int c = 1; c < nch; ++c)
            accj += s_pj[c];
        double hj = 0.0;
        for (int s = 0; s < t; ++s)
            hj = fma(wj[s], wj[s], hj);
        const double piv = ((kfun(kp.kind, 0.0, kp.sf2) - accj) - hj) + obs_noise; // (k(v_j, v_j): the distance is exactly 0)
        if (!(piv > 0.0) || !(piv <= DBL_MAX)) { // every workgroup comes to the same verdict from the same numbers
            if (blockIdx.x == 0 && threadIdx.x == 0)
                st->bad = 1; // (read by the next launch, k_sel_pick)
            return;
        }
        if (m < M) {
            double z = 0.0;
            for (int d = 0; d < kp.D; ++d) { // the difference is scaled, as k_build does (kbuild.hip)
                const double q = (Qt[(int64_t)d * ldq + m] - Qt[(int64_t)d * ldq + j]) * kp.inv_ell[d];
                z = fma(q, q, z);
            }
            double acc = part[m];
#pragma unroll 16
            for (int c = 1; c < nch; ++c) // ascending k
                acc += part[(int64_t)c * ldp + m];
            double h = 0.0;
#pragma unroll 4
            for (int s = 0; s < t; ++s)
                h = fma(W[m + (int64_t)s * ldw], wj[s], h);
            const double w = ((kfun(kp.kind, z, kp.sf2) - acc) - h) / sqrt(piv);
            W[m + (int64_t)t * ldw] = w;
            var[m] = var[m] - w * w;
            if (m == j)
                picked[m] = 1;
        }
    }
    double bv = 0.0;
    long long bi = -1;
    if (m < M && !(distinct && (picked[m] != 0 || m == j))) {
        bv = sel_score(rule, mu[m], var[m], var_add, param);
        bi = bv == bv ? m : -1; // (a NaN score is never a winner)
    }
    sel_best<SEL_FT>(sv, si, bv, bi);
    if (threadIdx.x == 0) {
        pairs[2 * blockIdx.x] = sv[0];
        pairs[2 * blockIdx.x + 1] = __longlong_as_double(si[0]);
    }
}

// One workgroup, behind k_sel_fold(r - 1): a failed pivot of round r - 1 -> fail = r; else, r < q, the pairs -> the pick of round r
__global__ __launch_bounds__(256) void k_sel_pick(SelState* __restrict__ st, const double* __restrict__ pairs, int npairs, int r, int q,
                                                  long long* __restrict__ idx, double* __restrict__ score)
{
    __shared__ double sv[256];
    __shared__ long long si[256];
    if (st->fail != 0)
        return;
    if (st->bad != 0) { // (uniform: every thread reads the same word)
        if (threadIdx.x == 0)
            st->fail = r;
        return;
    }
    if (r >= q)
        return;
    double bv = 0.0;
    long long bi = -1;
    for (int p = threadIdx.x; p < npairs; p += 256) {
        const double v = pairs[2 * p];
        const long long i = __double_as_longlong(pairs[2 * p + 1]);
        if (i >= 0 && (bi < 0 || v > bv || (v == bv && i < bi))) {
            bv = v;
            bi = i;
        }
    }
    sel_best<256>(sv, si, bv, bi);
    if (threadIdx.x == 0) {
        if (si[0] < 0) { // no eligible candidate (every score is NaN): this round cannot be played
            st->fail = r + 1;
            idx[r] = -1;
            score[r] = __longlong_as_double(0x7ff8000000000000LL);
            return;
        }
        st->j = si[0];
        idx[r] = si[0];
        score[r] = sv[0];
    }
}

void launch_sel_transpose(hipStream_t s, const double* Z, int64_t ld, int64_t N, int64_t M, double* Zt, int64_t ldz)
{
    if (N > 0 && M > 0)
        GPE_LAUNCH(k_sel_transpose, dim3((unsigned)((N + 31) / 32), (unsigned)((M + 31) / 32)), dim3(256), 0, s, Z, ld, N, M, Zt, ldz);
}

void launch_sel_score0(hipStream_t s, const SelRound& g)
{
    const int nwg = select_fold_groups(g.M);
    GPE_LAUNCH(k_sel_fold, dim3((unsigned)nwg), dim3(SEL_FT), 0, s, g.st, g.part, g.ldp, g.nch, g.Qt, g.ldq, g.M, *g.kp, g.W, g.ldw, g.wj, -1, g.var,
               g.mu, g.picked, g.rule, g.param, g.var_add, g.obs_noise, g.distinct, g.pairs);
    GPE_LAUNCH(k_sel_pick, dim3(1), dim3(256), 0, s, g.st, g.pairs, nwg, 0, g.q, g.idx, g.score);
}

void launch_sel_round(hipStream_t s, const SelRound& g, int t)
{
    const int nwg = select_fold_groups(g.M);
    GPE_LAUNCH(k_sel_gather, dim3((unsigned)((g.N + t + 255) / 256)), dim3(256), 0, s, g.st, g.Zt, g.ldz, g.N, g.W, g.ldw, t, g.zj, g.wj);
    GPE_LAUNCH(k_sel_colprod, dim3((unsigned)g.nrows), dim3(256), 0, s, g.st, g.plan, g.Zt, g.ldz, g.zj, g.part, g.ldp);
    GPE_LAUNCH(k_sel_fold, dim3((unsigned)nwg), dim3(SEL_FT), 0, s, g.st, g.part, g.ldp, g.nch, g.Qt, g.ldq, g.M, *g.kp, g.W, g.ldw, g.wj, t, g.var,
               g.mu, g.picked, g.rule, g.param, g.var_add, g.obs_noise, g.distinct, g.pairs);
    GPE_LAUNCH(k_sel_pick, dim3(1), dim3(256), 0, s, g.st, g.pairs, nwg, t + 1, g.q, g.idx, g.score);
}
