// potrf.hip — the serial piece of the blocked Cholesky (gfx950): the 64 x 64 diagonal block.
//
// Together with gemm.hip this replaces Eigen::LLT<MatrixXd>(K).matrixL()
// (src/limbo/model/gp.hpp:565) and the TriangularView solves (gp.hpp:260-261, :608-610, :620).
//
//   k_diag_full one workgroup: factor the diagonal block D = L11 L11^T (any jb <= 64) by the barrier rounds described below and
//               invert it; writes L11 in place and X^T = L11^-T (as Xt[k + 64 c] = X[c][k]) to a side buffer.  launch_diag sends
//               full blocks to k_diag(_b) instead: since round 2 a data-flow of seven specialised waves (diag_flow.h).
//   k_diag_inv  the inversion alone, batched over blocks (load(..., recompute = false) and
//               add_sample need the inverses of blocks they did not factor).
// The launches that start from such a block: potrf_panel.hip (k_diag, k_panel_step, k_panel256, k_upd_fused, k_head_copy) and
// potrf_tail.hip (k_tail, the ragged-block finish); potrf_tile.h is what the three files share.
//
// Everything below the diagonal block then is a matrix-core product with X (gemm.hip):
// L21 = A21 X^T, and the triangular sweeps become 64 x 64 mat-vecs with X / X^T (solve.hip).
//
// Factorisation.  The critical path of a Cholesky is the chain of N pivots
// (pivot -> rsqrt -> scale -> update of the next column), ~170 cycles each on this chip
// (tools/ubench.hip); everything here is arranged around it.  Thread (r, w): lane r = row,
// wave w owns the four-column groups g = 4q + w (columns 4g .. 4g+3), 16 doubles per thread.
// Round g: the owner wave first applies round g-1's rank-4 update to its four columns, then
// factors the 64 x 4 panel entirely inside the wave (pivot and multipliers broadcast with
// v_readlane, 1/sqrt by v_rsq_f64 + two Newton steps — no IEEE sqrt/div sequence on the chain),
// and publishes the four scaled columns through LDS; ONE barrier per four columns.  The other
// three waves meanwhile apply the previous rank-4 update to all their later columns; the owner's
// own non-critical columns are caught up one round later (4 LDS buffers keep that legal).
#include "potrf_tile.h"
#ifdef DIAG_TIMING // the stamps of k_diag_full's barrier rounds and inversion (k_diag's: potrf_panel.hip)
__device__ long long g_diag_arr[16][8]; // per round: arrival of waves 0-3 and of the inversion wave (4) at the closing barrier
__device__ long long g_diag_full_ts[32];
#endif
#if defined(DIAG_TIMING) && !defined(DIAG_NO_STAMPS) // (DIAG_NO_STAMPS: the arrays exist, the kernel is the shipped one)
#define ARR(G, w) do { if ((threadIdx.x & 63) == 0 && blockIdx.x == 0) g_diag_arr[G][w] = clock64(); } while (0)
#define TS(i) do { if (threadIdx.x == 0) g_diag_full_ts[i] = clock64(); } while (0)
#else
#define TS(i) do { } while (0)
#define ARR(G, w) do { } while (0)
#endif

// Scaling a column by 1/sqrt(p) with the shortest dependent chain (every fp64 op costs ~32 cycles
// of latency on the pivot chain): y0 = v_rsq_f64(p) is a ~1e-8-accurate seed; with
// eh = 1/2 - (p/2) y0^2 (= half the relative residual) the Newton-corrected factor is
// y = y0 (1 + eh) and a * y = fma(a*y0, eh, a*y0).  Chain: rsq -> mul -> fma -> fma.
// A second correction step is applied off the chain only to the stored inverse pivot `y`.
struct RsqScale {
    double y0, eh;
    __device__ __forceinline__ explicit RsqScale(double p)
    {
        y0 = __builtin_amdgcn_rsq(p);
        const double t = (0.5 * p) * y0;
        eh = fma(-t, y0, 0.5);
    }
    __device__ __forceinline__ double scale(double a) const
    {
        const double l = a * y0;
        return fma(l, eh, l);
    }
    // 1/sqrt(p) itself, one more Newton step (not on the critical path)
    __device__ __forceinline__ double inv(double p) const
    {
        double y = fma(y0, eh, y0);
        const double t = p * y;
        const double e = fma(-t, y, 1.0);
        return fma(0.5 * y, e, y);
    }
};

// a[qq][*] -= sum_e Lt[r][e] * Lt[c][e] for this thread's column groups qq with 4 qq + w >= gmin
// (Lt: one round's four scaled columns, Lt[row * 4 + e])
static __device__ __forceinline__ void rank4_update(double (&a)[4][4], const double* __restrict__ Lt, int r, int w,
                                                    int gmin, int qlo)
{
    const double m0 = Lt[r * 4 + 0], m1 = Lt[r * 4 + 1], m2 = Lt[r * 4 + 2], m3 = Lt[r * 4 + 3];
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
        if (qq < qlo || 4 * qq + w < gmin)
            continue; // wave-uniform
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double* lc = Lt + (16 * qq + 4 * w + e) * 4; // wave-uniform address: LDS broadcast
            double v = a[qq][e];
            v = fma(-m0, lc[0], v);
            v = fma(-m1, lc[1], v);
            v = fma(-m2, lc[2], v);
            v = fma(-m3, lc[3], v);
            a[qq][e] = v;
        }
    }
}

template <int G>
struct DiagRound {
    static __device__ __forceinline__ void run(double (&a)[4][4], double* __restrict__ Ltb, double* __restrict__ invd,
                                               int* __restrict__ sbad, int r, int w, double* __restrict__ Ls)
    {
        DiagRound<G - 1>::run(a, Ltb, invd, sbad, r, w, Ls);
        constexpr int q = G >> 2, own = G & 3, c0 = 4 * G;
        double* Lt = Ltb + (G & 3) * (NB * 4);
        const double* Lp = Ltb + ((G + 3) & 3) * (NB * 4); // round G-1
        const double* Lpp = Ltb + ((G + 2) & 3) * (NB * 4); // round G-2
        if (w == own) {
            if (G > 0) {
                // critical: round G-1's update on this group's four columns only
                const double m0 = Lp[r * 4 + 0], m1 = Lp[r * 4 + 1], m2 = Lp[r * 4 + 2], m3 = Lp[r * 4 + 3];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double* lc = Lp + (c0 + e) * 4;
                    double v = a[q][e];
                    v = fma(-m0, lc[0], v);
                    v = fma(-m1, lc[1], v);
                    v = fma(-m2, lc[2], v);
                    v = fma(-m3, lc[3], v);
                    a[q][e] = v;
                }
            }
            double a0 = a[q][0], a1 = a[q][1], a2 = a[q][2], a3 = a[q][3];
            // column c0
            const double p0 = bcast_lane(a0, c0);
            const RsqScale s0(p0);
            const double l0 = s0.scale(a0);
            a1 = fma(-l0, bcast_lane(l0, c0 + 1), a1);
            // column c0+1
            const double p1 = bcast_lane(a1, c0 + 1);
            const RsqScale s1(p1);
            a2 = fma(-l0, bcast_lane(l0, c0 + 2), a2);
            a3 = fma(-l0, bcast_lane(l0, c0 + 3), a3);
            const double l1 = s1.scale(a1);
            a2 = fma(-l1, bcast_lane(l1, c0 + 2), a2);
            // column c0+2
            const double p2 = bcast_lane(a2, c0 + 2);
            const RsqScale s2(p2);
            a3 = fma(-l1, bcast_lane(l1, c0 + 3), a3);
            const double l2 = s2.scale(a2);
            a3 = fma(-l2, bcast_lane(l2, c0 + 3), a3);
            // column c0+3
            const double p3 = bcast_lane(a3, c0 + 3);
            const RsqScale s3(p3);
            const double l3 = s3.scale(a3);
            const double y0 = s0.inv(p0), y1 = s1.inv(p1), y2 = s2.inv(p2), y3 = s3.inv(p3);
            a[q][0] = l0;
            a[q][1] = l1;
            a[q][2] = l2;
            a[q][3] = l3;
            Lt[r * 4 + 0] = l0;
            Lt[r * 4 + 1] = l1;
            Lt[r * 4 + 2] = l2;
            Lt[r * 4 + 3] = l3;
            if (Ls) { // the finished columns, for the inversion pipeline (XPipe32)
                Ls[r * XS + c0 + 0] = l0;
                Ls[r * XS + c0 + 1] = l1;
                Ls[r * XS + c0 + 2] = l2;
                Ls[r * XS + c0 + 3] = l3;
            }
            if (r == 0) {
                invd[c0 + 0] = y0;
                invd[c0 + 1] = y1;
                invd[c0 + 2] = y2;
                invd[c0 + 3] = y3;
                // first non-positive pivot (the reference never checks LLT::info(), gp.hpp:565)
                int bad = 0;
                if (!(p3 > 0.0))
                    bad = c0 + 4;
                if (!(p2 > 0.0))
                    bad = c0 + 3;
                if (!(p1 > 0.0))
                    bad = c0 + 2;
                if (!(p0 > 0.0))
                    bad = c0 + 1;
                if (bad != 0 && *sbad == 0)
                    *sbad = bad;
            }
        }
        else {
            if (G > 1 && w == ((G - 1) & 3)) // last round's owner catches up on round G-2
                rank4_update(a, Lpp, r, w, G, 0);
            if (G > 0)
                rank4_update(a, Lp, r, w, G, 0);
        }
        ARR(G, w);
        __syncthreads();
        if (G < 16)
            TS(10 + G);
    }
};
template <>
struct DiagRound<-1> {
    static __device__ __forceinline__ void run(double (&)[4][4], double*, double*, int*, int, int, double*) {}
};

// (Round 2 also built 8-column rounds here — half the barriers and publishes, optionally with a 1/p update chain — and
// measured them neutral, profiles/r02_diag_rounds.log; the data-flow form in diag_flow.h replaced that line of attack and
// the code was removed.)

#define DIAG_COL(q, e, w) (16 * (q) + 4 * (w) + (e))
#define DIAG_RUN(a, Ltb, invd, sbad, r, w, Ls) DiagRound<15>::run(a, Ltb, invd, sbad, r, w, Ls)

// ---- inversion of the 64 x 64 lower-triangular L (in LDS, Ls[row * XS + col]) --------------------
// acc[n] += sum_{k < 16} P[i0 + i][pk0 + k] * Q[qk0 + k][j0 + 4 n + j]   (16 x 16 x 16, n in [n0, n1))
static __device__ __forceinline__ void mm16(const double* __restrict__ P, int i0, int pk0, const double* __restrict__ Q,
                                            int qk0, int j0, double (&acc)[4], int n0, int n1, int lane)
{
    const int ai = i0 + (lane & 15), kq = lane >> 4, bj = j0 + (lane & 3);
#pragma unroll
    for (int ks = 0; ks < 16; ks += 4) {
        const double av = P[ai * XS + pk0 + ks + kq];
#pragma unroll
        for (int n = 0; n < 4; ++n)
            if (n >= n0 && n < n1)
                acc[n] = mfma4(av, Q[(qk0 + ks + kq) * XS + bj + 4 * n], acc[n]);
    }
}
// D[i0 + row][j0 + col] = sign * acc   (result layout of v_mfma_f64_4x4x4_4b, see gemm.hip)
static __device__ __forceinline__ void st16(double* __restrict__ D, int i0, int j0, const double (&acc)[4], int n0,
                                            int n1, double sign, int lane)
{
    const int row = i0 + 4 * ((lane >> 2) & 3) + (lane >> 4), col = j0 + (lane & 3);
#pragma unroll
    for (int n = 0; n < 4; ++n)
        if (n >= n0 && n < n1)
            D[row * XS + col + 4 * n] = sign * acc[n];
}

// level 2: X[32:64, 0:32] = -X22 (L21 X11) given the two 32 x 32 diagonal inverses in Xs, one
// 16 x 16 block per wave; 256 threads, ends with a barrier
static __device__ __forceinline__ void invert_level2(const double* __restrict__ Ls, double* __restrict__ Xs,
                                                     double* __restrict__ Ts)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ib = 2 + (w >> 1), jb = w & 1;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int kb = jb; kb < 2; ++kb) // T = L_21 X_11, X_11 lower
        mm16(Ls, 16 * ib, 16 * kb, Xs, 16 * kb, 16 * jb, acc, 0, 4, lane);
    st16(Ts, 16 * ib, 16 * jb, acc, 0, 4, 1.0, lane);
    __syncthreads();
    double acc2[4] = {0.0, 0.0, 0.0, 0.0};
    for (int kb = 2; kb <= ib; ++kb) // X_21 = -X_22 T, X_22 lower
        mm16(Xs, 16 * ib, 16 * kb, Ts, 16 * kb, 16 * jb, acc2, 0, 4, lane);
    st16(Xs, 16 * ib, 16 * jb, acc2, 0, 4, -1.0, lane);
    __syncthreads();
}

// Ls: L (lower, zeros above).  invd[j] = 1 / L[j][j].  Xs <- L^-1 (zeros above).  Ts: scratch.
// All 256 threads; ends with a barrier.
static __device__ __forceinline__ void invert_L64(const double* __restrict__ Ls, const double* __restrict__ invd,
                                                  double* __restrict__ Xs, double* __restrict__ Ts)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int e = threadIdx.x; e < NB * XS; e += 256)
        Xs[e] = 0.0;
    __syncthreads();
    TS(4);
    { // level 0: the four 16 x 16 diagonal blocks, wave w -> block w, lane (mod 16) = column of X
        const int b0 = 16 * w, c = lane & 15;
        double x[16];
#pragma unroll
        for (int j = 0; j < 16; ++j)
            x[j] = (j == c) ? 1.0 : 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            x[j] *= invd[b0 + j];
#pragma unroll
            for (int i = j + 1; i < 16; ++i)
                x[i] = fma(-Ls[(b0 + i) * XS + b0 + j], x[j], x[i]);
        }
        if (lane < 16) {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                Xs[(b0 + j) * XS + b0 + c] = x[j];
        }
    }
    __syncthreads();
    TS(5);
    { // level 1: blocks (1,0) and (3,2):  X_ib,jb = -X_ib,ib (L_ib,jb X_jb,jb); two waves per block
        const int t = w >> 1, h = w & 1, ib = 2 * t + 1, jb = 2 * t;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        mm16(Ls, 16 * ib, 16 * jb, Xs, 16 * jb, 16 * jb, acc, 2 * h, 2 * h + 2, lane);
        st16(Ts, 16 * ib, 16 * jb, acc, 2 * h, 2 * h + 2, 1.0, lane);
        __syncthreads();
        double acc2[4] = {0.0, 0.0, 0.0, 0.0};
        mm16(Xs, 16 * ib, 16 * ib, Ts, 16 * ib, 16 * jb, acc2, 2 * h, 2 * h + 2, lane);
        st16(Xs, 16 * ib, 16 * jb, acc2, 2 * h, 2 * h + 2, -1.0, lane);
    }
    __syncthreads();
    TS(6);
    invert_level2(Ls, Xs, Ts);
    TS(7);
}

// Xt[k + 64 c] = X[c][k]
static __device__ __forceinline__ void store_Xt(const double* __restrict__ Xs, double* __restrict__ Xt)
{
    for (int e = threadIdx.x; e < NB * NB; e += 256)
        Xt[e] = Xs[(e >> 6) * XS + (e & 63)];
}

// Full-inverse form (any jb <= 64): the three-launch panel step and its GEMM consumers need all of X.
__global__ __launch_bounds__(256) void k_diag_full(double* __restrict__ A, int64_t lda, int jb, double* __restrict__ Xt,
                                              int* __restrict__ info, int64_t goff, const BatchTab* __restrict__ bt)
{
    BT_REBASE(bt, A);
    BT_REBASE(bt, Xt);
    BT_REBASE(bt, info);
    __shared__ __attribute__((aligned(16))) double Ls[NB * XS];
    __shared__ __attribute__((aligned(16))) double Xs[NB * XS];
    __shared__ __attribute__((aligned(16))) double Ts[NB * XS];
    __shared__ __attribute__((aligned(16))) double Ltb[DIAG_LTB];
    __shared__ double invd[NB];
    __shared__ int sbad;
    const int r = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (threadIdx.x == 0)
        sbad = 0;
    double a[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = DIAG_COL(q, e, w);
            // only the lower triangle of A is meaningful; a short block is padded with the identity
            a[q][e] = (r < jb && c < jb) ? ((c <= r) ? A[r + (int64_t)c * lda] : 0.0) : ((r == c) ? 1.0 : 0.0);
        }
    TS(0);
    __syncthreads();
    TS(1);
    DIAG_RUN(a, Ltb, invd, &sbad, r, w, nullptr);
    TS(2);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = DIAG_COL(q, e, w);
            const double v = (c <= r) ? a[q][e] : 0.0;
            Ls[r * XS + c] = v;
            if (r < jb && c <= r)
                A[r + (int64_t)c * lda] = v;
        }
    if (threadIdx.x == 0 && sbad != 0 && sbad <= jb && *info == 0)
        *info = (int)(goff + sbad);
    __syncthreads();
    TS(3);
    invert_L64(Ls, invd, Xs, Ts);
    store_Xt(Xs, Xt);
    TS(8);
}

#ifdef DIAG_TIMING
void dump_diag_full_timing()
{
    {
        long long a[16][8];
        (void)hipMemcpyFromSymbol(a, HIP_SYMBOL(g_diag_arr), sizeof(a));
        printf("arrival at the closing barrier of round G, cycles after the previous barrier's last arrival (waves 0-3 factor, X = inversion wave; * = owner):\n");
        long long prev = 0;
        for (int G = 0; G < 16; ++G) {
            long long last = 0;
            for (int w = 0; w < 5; ++w)
                last = a[G][w] > last ? a[G][w] : last;
            if (G > 0) {
                printf("  G=%2d:", G);
                for (int w = 0; w < 5; ++w)
                    printf(" %s%6lld%s", w == 4 ? "X" : "w", a[G][w] - prev, w == (G & 3) ? "*" : " ");
                printf("\n");
            }
            prev = last;
        }
    }
    long long h[32];
    hipMemcpyFromSymbol(h, HIP_SYMBOL(g_diag_full_ts), sizeof(h));
    printf("k_diag_full cycles (factor waves): load %lld | rounds %lld | writeL %lld | total %lld\n", h[1] - h[0], h[2] - h[1],
           h[3] - h[2], h[3] - h[0]);
    printf("rounds:");
    for (int g = 0; g < 16; ++g)
        printf(" %lld", h[10 + g] - (g ? h[9 + g] : h[1]));
    printf("\n");
}
#endif
void launch_diag(hipStream_t s, double* A, int64_t lda, int jb, double* Xt, int* info, int64_t goff, int half_form)
{
    if (half_form && jb == NB)
    {
        if (g_batch.bt)
            GPE_LAUNCH(k_diag_b, dim3(1, 1, g_batch.G), dim3(DIAG_THREADS), 0, s, A, lda, Xt, info, goff, g_batch.bt);
        else
            GPE_LAUNCH(k_diag, dim3(1), dim3(DIAG_THREADS), 0, s, A, lda, Xt, info, goff);
    }
    else
        GPE_LAUNCH(k_diag_full, dim3(1, 1, g_batch.G), dim3(256), 0, s, A, lda, jb, Xt, info, goff, g_batch.bt);
}

// inverses of the diagonal blocks of an existing factor: block b at L[64 b, 64 b]
__global__ __launch_bounds__(256) void k_diag_inv(const double* __restrict__ L, int64_t ldl, int64_t N, int64_t b0,
                                                  double* __restrict__ Xt_all)
{
    __shared__ __attribute__((aligned(16))) double Ls[NB * XS];
    __shared__ __attribute__((aligned(16))) double Xs[NB * XS];
    __shared__ __attribute__((aligned(16))) double Ts[NB * XS];
    __shared__ double invd[NB];
    const int64_t b = b0 + blockIdx.x;
    const int64_t j0 = b * NB;
    const int jb = (int)((N - j0 < NB) ? N - j0 : NB);
    const double* L11 = L + j0 + j0 * ldl;
    for (int e = threadIdx.x; e < NB * NB; e += 256) {
        const int r = e & 63, c = e >> 6;
        double v = 0.0;
        if (r < jb && c < jb)
            v = (c <= r) ? L11[r + (int64_t)c * ldl] : 0.0;
        else if (r == c)
            v = 1.0;
        Ls[r * XS + c] = v;
        if (r == c)
            invd[r] = 1.0 / v;
    }
    __syncthreads();
    invert_L64(Ls, invd, Xs, Ts);
    store_Xt(Xs, Xt_all + b * (NB * NB));
}

void launch_diag_inv(hipStream_t s, const double* L, int64_t ldl, int64_t N, int64_t b0, int64_t nblocks,
                     double* Xt_all)
{
    if (nblocks <= 0)
        return;
    GPE_LAUNCH(k_diag_inv, dim3((unsigned)nblocks), dim3(256), 0, s, L, ldl, N, b0, Xt_all);
}
