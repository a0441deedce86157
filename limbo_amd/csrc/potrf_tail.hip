// potrf_tail.hip — the data-flow launch of the blocked Cholesky (gfx950), k_tail(_g, _b), with its chain workgroup and dispatch
// order, and what finishes a ragged order's last block behind it (k_ragged_*).  Each is described where it is defined.
#include "potrf_tile.h"
#include <array>
#include <map>
#include <mutex>
#include <vector>
#ifdef DIAG_TIMING
__device__ long long g_tail_ts[64][4]; // k_tail, the diagonal workgroup of column c: updates done | solved | factoring | factored
__device__ long long g_tail_cyc[64][4]; // ... the same stamps in shader-clock cycles (clock64): cycles / wall time = the clock the CU ran at
#define TTS(c, i) do { if (threadIdx.x == 0 && (c) < 64) { g_tail_ts[(c)][(i)] = wall_clock64(); g_tail_cyc[(c)][(i)] = clock64(); } } while (0)
__device__ long long g_tail_ts2[64][12]; // ... inside its two-phase solve: X11/L21 seen | phase A done | X22 seen | X22 in LDS | Y2 written | done
#define TTS2(x, on, i) do { if ((on) && threadIdx.x == 0 && ((x).R0 - (x).p0) / NB < 64) g_tail_ts2[((x).R0 - (x).p0) / NB][(i)] = wall_clock64(); } while (0)
#else
#define TTS(c, i) do { } while (0)
#define TTS2(x, on, i) do { } while (0)
#endif

// ---------------------------------------------------------------------------------------------
// k_tail (round 3) — the LAST T <= 1024 columns of the factorisation (or all of it when N <= 1024) as ONE launch: a tiled
// data-flow Cholesky.  The last four outer panels of N = 4096 hold 1.5 % of the flops and took 20 % of the time: each is a
// k_panel256 of 4-16 strips (~48 us: three diagonal blocks one after the other), a fused update for a handful of tiles
// (~16 us) and two launch boundaries, although the whole remaining matrix — 136 tiles of 64 x 64 — fits on the chip with one
// workgroup per tile.  Here workgroup (b, c) owns tile (b, c) of the lower triangle (b >= c; row strip nt = the right-hand-side
// rows) and keeps it in registers for the whole launch:
//   steps s = 0 .. c-1:  tile -= L(b, s) L(c, s)^T, both operands polled from the owners of those tiles (PolledTile; the next
//                        step's operands are asked for before this step's product)
//   step c, b == c:      the diagonal block is complete: factor it (diag_flow), its inverse leaves in polled quarters
//   step c, b >  c:      L(b, c) = tile X_c^T in the half-block form, in two phases (tail_tile_solve; the chain workgroup:
//                        tail_chain_updates_and_crossing), published in two halves
// Workgroups are numbered column by column, the diagonal tile first: every wait is for a lower-numbered workgroup.  The chain
// diag(c) -> X_c -> L(c+1, c) -> last update of tile (c+1, c+1) -> diag(c+1) is what k_panel256's is, without the fused
// updates and launch boundaries in between.  Polled buffers: LP (a 4096-double slot per tile, blockIdx order) and SP (3072 doubles
// per diagonal block), all-ones when the launch starts; every workgroup arms its own slot of the OTHER pair for the next launch.
// ---------------------------------------------------------------------------------------------
// Round 4: the launch is no longer tied to the END of the matrix.  A "tall" launch factors the nt tile columns t0 .. t1 of a
// panel that has nfull >= nt full row strips under its first row (rows t0 .. N64) plus the right-hand-side strip: the whole
// 1536-column head of an N = 4096 factorisation is one such launch (24 tile columns x 64 row strips), one k = 1536 update and
// the closing launch (nfull = nt) follow — no 256-column panels, no look-ahead stream.  Batched (k_tail_b): the tiles of G
// members interleave in the 1-D grid (id = tile * G + member), so that the G chains advance side by side and every wait is
// still for a lower-numbered workgroup.
struct TailArgs {
    double* A;
    int64_t lda, t0; // the launch starts at row / column t0
    int nt, nb;      // tile columns; row strips (nfull, + 1 for the right-hand-side rows)
    int nfull;       // full 64-row strips (>= nt; == nt for the closing launch)
    int rhs_rows;
    double* Xt;      // inverse of the diagonal block at t0 (the others follow at + 4096 each)
    int* info;
    double *LP, *SP, *LPn, *SPn;
    int spin_limit;
    const int* order; // dispatch order: workgroup w works on tile (b, c) = (order[2 w], order[2 w + 1]); null: column by column
    // gen (Xg != null): the launch GENERATES its tiles of K from the samples instead of reading them from A — the kernel matrix
    // is never written for the columns this launch factors (kernel/kernel.hpp:81-84 with the functors of kfun_fast.h, the
    // pair formula and summation order of kbuild.hip); rows >= Ns of the last strip are obs_mean's rows, read from Om
    const double* Xg; // SoA samples, Xg[d * ldx + i]
    int64_t ldx, Ns;  // Ns: samples (rows below Ns in the last strip: right-hand sides)
    const double* Om; // obs_mean, Om[i + p * ldom]
    int64_t ldom;
    double* Al;       // optional: the backward sweep's output, pre-filled with its sentinel here (what the build launch does)
    int64_t ldal;
    int P;
};
// LDS of a k_tail workgroup: two pairs of operand tiles [A0 | B0 | A1 | B1] (40 KB each: all of the CU's 160 KB) for the pipelined
// products of the update loop; behind it the carve of the solve and the factorisation (CH_*, further down)
#define TAIL_LDS_DOUBLES (4 * NB * PS)
static_assert(TAIL_LDS_DOUBLES >= NB * XS + 3 * NB * PS && TAIL_LDS_DOUBLES * 8 <= 160 * 1024, "k_tail LDS carve");
static __device__ __forceinline__ int tail_tile_id(int nb, int b, int c) { return c * nb - (c * (c - 1)) / 2 + (b - c); }

// element it of a thread's tile slice: global row I (clamped into the strip by the caller), global columns J0 + 2 it
static __device__ __forceinline__ void tail_gen_tile(const TailArgs& a, const KParams* __restrict__ kp, int64_t I, int64_t J0,
                                                     double (&out)[8])
{
    if (I >= a.Ns) { // a right-hand-side row: obs_mean^T
        const double* om = a.Om + (I - a.Ns) * a.ldom;
#pragma unroll
        for (int it = 0; it < 8; ++it)
            out[it] = om[J0 + 2 * it];
        return;
    }
    double z[8];
#pragma unroll
    for (int it = 0; it < 8; ++it)
        z[it] = 0.0;
    const int D = kp->D;
    for (int d = 0; d < D; ++d) {
        const double* xr = a.Xg + (int64_t)d * a.ldx;
        const double xi = xr[I], ie = kp->inv_ell[d];
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const double q = (xi - xr[J0 + 2 * it]) * ie;
            z[it] = fma(q, q, z[it]);
        }
    }
    const int kind = kp->kind;
    const double sf2 = kp->sf2, da = kp->diag_add;
#pragma unroll
    for (int it = 0; it < 8; ++it)
        out[it] = kfun_fast_rt(kind, z[it], sf2) + (I == J0 + 2 * it ? da : 0.0);
}

// ---- k_tail's chain workgroup (round 5) ----------------------------------------------------------------------------------------
// Stamps (tools/kbench_t, profiles/r05_chain_stamps.log) showed that a hop of the chain is NOT "panel wave, then the crossing":
// three loops of about the same length go round at once —
//   (1) panel wave of block c-1 ends -> X22 visible -> phase B of block c's crossing -> first pivot -> panel wave of block c ends
//   (2) second half of L(c-1, c-2) published -> the LAST update step of workgroup c (it needs that tile) -> phase A -> phase B up to
//       the publication of L(c, c-1)'s second half
//   (3) X11 / L21 of block c-1 visible -> phase A -> phase B -> first pivot -> ... -> X11 / L21 of block c
// and every stage in them is tens of matrix-core instructions between barriers: two waves share a SIMD's matrix pipe, a
// 64 x 64 x 32 product is 0.85 us of it, the five products of a crossing 3 us.  So, here:
//  * products only over what is not zero and not thrown away: Y Y^T and L L^T feed the LOWER triangle of the diagonal block —
//    40 of its 64 units of 16 x 4, five per wave (syrk40) —, X11 and X22 are triangular (tri_solve32 stops at the diagonal and
//    pairs the waves of a SIMD so that their k ranges add up to the same);
//  * no layout conversions and no staging on the path: the diagonal block's lower triangle lives in the matrix-core accumulators
//    from the moment the workgroup starts (a2v = -tile) to the factorisation — every update of the loop and both halves of the
//    crossing add to that ONE chain, and what the factorisation reads is its negative, stored once (syrk40_store_neg); the tile
//    (c, c-1) sits in LDS in the layout the solve multiplies ([kk][i]) and the loop's sum is subtracted from it in place;
//  * the last update step half by half: BOTH of its tiles, L(c-1, c-2) and L(c, c-2), are published in two halves 3 us apart —
//    the k = 0..31 halves of both products run before the second halves arrive, 1.4 us of matrix-core time is left behind them;
//  * results go to a scratch block nobody is reading (no write-after-read barriers); the chain workgroup watches ITS OWN words of
//    the polled quarters and tiles without a pause (chain_watch; the last step's two tiles in ONE round trip: chain_watch2) —
//    one workgroup at a time is there, and the launch is waiting for it.
//    (Measured and dropped: diag_flow reading the block from one buffer and publishing L into another, which saves the barrier
//    behind its waves' first loads — the panel wave then runs 0.5 us longer per block, 6.97 against 6.44 us, 1.160 against 1.154 ms.)
// LDS (doubles), two halves of 10240 = the two operand pairs of the update loop; the LAST step uses pair 0:
//   pair 1: T [kk][i] (5120) | X11 (stride 34, 1088) | L21 (stride 34, 1088)
//   pair 0: opA | opB of the last step; behind barrier A1: D (64 x XS) | H | invd | sy | Xw (Ys = Y1 / Y2 lies inside Xw) | X22
#define CH_T 10240
#define CH_X11 (CH_T + NB * PS)
#define CH_LD (CH_X11 + 32 * 34)
#define CH_D 0
#define CH_AUX (NB * XS)
#define CH_YS (CH_AUX + 1096)
#define CH_X22 (CH_AUX + 1096 + DIAG_XW_DOUBLES)
static_assert(CH_X22 + 32 * 34 <= CH_T && CH_YS + 32 * PS <= CH_X22 && CH_LD + 32 * 34 <= 4 * NB * PS, "chain workgroup LDS carve");

// acc[u] += the wave's five 16 x 4 units of the lower triangle of Aop Aop^T over k in [ak0, ak0 + KLEN)  (Aop: [kk][i], stride PS)
//   waves 0..3: column block j1 = w (columns 4w ..), row blocks 0..3 -> u = 0..3;  column block 15 - w, row block 3 -> u = 4
//   waves 4..7: column block j1 = w, row blocks 1..3 -> u = 0..2;  column block 15 - w, row blocks 2, 3 -> u = 3, 4
template <int KLEN>
static __device__ __forceinline__ void syrk40(const double* __restrict__ Aop, int ak0, int wave, int lane, double (&acc)[5])
{
    const int r16 = lane & 15, kq = lane >> 4, c4 = lane & 3;
    const int j1 = wave, j2 = 15 - wave;
    if (wave < 4) {
#pragma unroll
        for (int ks = 0; ks < KLEN; ks += 4) {
            const double* row = Aop + (ak0 + ks + kq) * PS;
            const double a0 = row[r16], a1 = row[16 + r16], a2 = row[32 + r16], a3 = row[48 + r16];
            const double b1 = row[4 * j1 + c4], b2 = row[4 * j2 + c4];
            acc[0] = mfma4(a0, b1, acc[0]);
            acc[1] = mfma4(a1, b1, acc[1]);
            acc[2] = mfma4(a2, b1, acc[2]);
            acc[3] = mfma4(a3, b1, acc[3]);
            acc[4] = mfma4(a3, b2, acc[4]);
        }
    }
    else {
#pragma unroll
        for (int ks = 0; ks < KLEN; ks += 4) {
            const double* row = Aop + (ak0 + ks + kq) * PS;
            const double a1 = row[16 + r16], a2 = row[32 + r16], a3 = row[48 + r16];
            const double b1 = row[4 * j1 + c4], b2 = row[4 * j2 + c4];
            acc[0] = mfma4(a1, b1, acc[0]);
            acc[1] = mfma4(a2, b1, acc[1]);
            acc[2] = mfma4(a3, b1, acc[2]);
            acc[3] = mfma4(a2, b2, acc[3]);
            acc[4] = mfma4(a3, b2, acc[4]);
        }
    }
}
// The eight columns (of a 32-column half) a wave's triangular products compute: waves w and w + 4 share a SIMD (dev.h) and get
// 0 | 24 and 8 | 16 — their k ranges, hn + 8 each, add up to 40 on every SIMD
static __host__ __device__ __forceinline__ int tri_solve_cols(int wave)
{
    const int hq = wave >> 1;
    return hq == 0 ? 0 : (hq == 1 ? 8 : (hq == 2 ? 24 : 16));
}
// y[m][n] = sum_{k <= column} Aop[ak0 + k][wm + 16 m + ..] X[column][k] for the wave's columns hn + 4 n + ..: X (32 x 32, row-major,
// stride 34) is lower triangular, the k loop stops at the wave's last column
static __device__ __forceinline__ void tri_solve32(const double* __restrict__ Aop, int ak0, const double* __restrict__ X, int wm,
                                                   int hn, int lane, double (&y)[2][2])
{
    const int ar = wm + (lane & 15), bc = hn + (lane & 3), kq = lane >> 4;
#pragma unroll
    for (int ks = 0; ks < 32; ks += 4) {
        if (ks >= hn + 8) // (wave-uniform)
            break;
        double af[2], bf[2];
#pragma unroll
        for (int m = 0; m < 2; ++m)
            af[m] = Aop[(ak0 + ks + kq) * PS + ar + 16 * m];
#pragma unroll
        for (int n = 0; n < 2; ++n)
            bf[n] = X[(bc + 4 * n) * 34 + ks + kq];
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int m = 0; m < 2; ++m)
                y[m][n] = mfma4(af[m], bf[n], y[m][n]);
    }
}

// The chain workgroup watches ITS OWN words of a polled block (device scope, no pause) until none shows the pattern: one look at
// poll_one's word, a pause and a second fetch of the own words are 0.5 us between "visible" and "seen" — on the chain.
template <int NW, int STRIDE = 512> // word q of a thread lies STRIDE words behind word q - 1
static __device__ __forceinline__ void chain_watch(const unsigned long long* __restrict__ p, unsigned long long (&b)[NW], int spin_limit,
                                                   int* __restrict__ info)
{
    static_assert(NW == 2 || NW == 4, "written out: the words stay in registers");
    const unsigned long long SENT = ~0ull;
    int spins = 0;
    if constexpr (NW == 4) {
        while (b[0] == SENT || b[1] == SENT || b[2] == SENT || b[3] == SENT) {
            if (++spins > spin_limit) {
                info[2] = 1;
                break;
            }
            if (b[0] == SENT) b[0] = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (b[1] == SENT) b[1] = __hip_atomic_load(p + STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (b[2] == SENT) b[2] = __hip_atomic_load(p + 2 * STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (b[3] == SENT) b[3] = __hip_atomic_load(p + 3 * STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    else {
        while (b[0] == SENT || b[1] == SENT) {
            if (++spins > spin_limit) {
                info[2] = 1;
                break;
            }
            if (b[0] == SENT) b[0] = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (b[1] == SENT) b[1] = __hip_atomic_load(p + STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    asm volatile("" ::: "memory");
}
// ... two blocks at once (four words of each): one round trip covers both
static __device__ __forceinline__ void chain_watch2(const unsigned long long* __restrict__ pa, unsigned long long (&a)[4],
                                                    const unsigned long long* __restrict__ pb, unsigned long long (&b)[4], int spin_limit,
                                                    int* __restrict__ info)
{
    const unsigned long long SENT = ~0ull;
    constexpr int STRIDE = 8 * NB;
    int spins = 0;
    while (a[0] == SENT || a[1] == SENT || a[2] == SENT || a[3] == SENT || b[0] == SENT || b[1] == SENT || b[2] == SENT || b[3] == SENT) {
        if (++spins > spin_limit) {
            info[2] = 1;
            break;
        }
        if (a[0] == SENT) a[0] = __hip_atomic_load(pa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (a[1] == SENT) a[1] = __hip_atomic_load(pa + STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (a[2] == SENT) a[2] = __hip_atomic_load(pa + 2 * STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (a[3] == SENT) a[3] = __hip_atomic_load(pa + 3 * STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (b[0] == SENT) b[0] = __hip_atomic_load(pb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (b[1] == SENT) b[1] = __hip_atomic_load(pb + STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (b[2] == SENT) b[2] = __hip_atomic_load(pb + 2 * STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (b[3] == SENT) b[3] = __hip_atomic_load(pb + 3 * STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("" ::: "memory");
}
// acc = -(the wave's units of a 64 x 64 block held row-major with stride XS) / the block's units = -acc  (syrk40's layout)
static __host__ __device__ __forceinline__ void syrk40_units(int wave, int q, int& i, int& j)
{
    if (wave < 4) {
        i = q < 4 ? q : 3;
        j = q < 4 ? wave : 15 - wave;
    }
    else {
        i = q < 3 ? q + 1 : q - 1;
        j = q < 3 ? wave : 15 - wave;
    }
}
static __device__ __forceinline__ void syrk40_load_neg(const double* __restrict__ Dl, int wave, int lane, double (&acc)[5])
{
    const int drow = 4 * ((lane >> 2) & 3) + (lane >> 4), dcol = lane & 3;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        int i, j;
        syrk40_units(wave, q, i, j);
        acc[q] = -Dl[(16 * i + drow) * XS + 4 * j + dcol];
    }
}
static __device__ __forceinline__ void syrk40_store_neg(double* __restrict__ Dl, int wave, int lane, const double (&acc)[5])
{
    const int drow = 4 * ((lane >> 2) & 3) + (lane >> 4), dcol = lane & 3;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        int i, j;
        syrk40_units(wave, q, i, j);
        Dl[(16 * i + drow) * XS + 4 * j + dcol] = -acc[q];
    }
}

// The chain workgroup of column c >= 1 from "tiles (c, c-1) and (c, c) loaded" (cl, cv: lane = row layout) to "the diagonal block is
// complete in lds + CH_D" (a barrier away from the factorisation); L(c, c-1) is left in lds + CH_T for the matrix.
static __device__ __forceinline__ void tail_chain_updates_and_crossing(const TailArgs& a, const P256& x, double* __restrict__ lds,
                                                                       const int c, const double (&cl)[8], const double (&cv)[8])
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 16; // a 64 x 64 product's wave tile
    const int hn = tri_solve_cols(wave);
    const int crow = wm + (lane & 31), ccol = wn + (lane >> 5);
    const int drow = 4 * ((lane >> 2) & 3) + (lane >> 4), dcol = lane & 3;
    double* const T = lds + CH_T;
    double* const X11 = lds + CH_X11;
    double* const Ld = lds + CH_LD;
    double* const Dl = lds + CH_D;
    double* const Ys = lds + CH_YS;
    double* const X22 = lds + CH_X22;
    const double* Sq = a.SP + (int64_t)(c - 1) * 3072;
    double* pub = a.LP + (int64_t)tail_tile_id(a.nb, c, c - 1) * (NB * NB);
    const unsigned long long* Sp = reinterpret_cast<const unsigned long long*>(Sq) + threadIdx.x;
    // The diagonal block's lower triangle lives in the matrix-core accumulators from here to the factorisation: a2v = -(tile) now,
    // + every product of the loop and of the crossing, and -a2v is what the factorisation reads.  (Through LDS once, here, where
    // nothing is waiting: the tile was loaded / generated in the lane = row layout.)
    double a2v[5];
#pragma unroll
    for (int it = 0; it < 8; ++it)
        lds[crow * XS + ccol + 2 * it] = cv[it];
    __syncthreads();
    syrk40_load_neg(lds, wave, lane, a2v);
    __syncthreads(); // (the loop's first operands land in the same place)
    unsigned long long xb[4]; // X11: e, e + 512; L21: 1024 + e, 1024 + e + 512
    if (c > 1) {
        // Steps s < c-1: tile (c, c-1) -= L(c, s) L(c-1, s)^T, tile (c, c) -= L(c, s) L(c, s)^T.  Software-pipelined over two pairs of
        // operand buffers (the operands of step s+1 are on their way under the products of step s: one barrier a step); the pair
        // alternates so that the LAST step uses pair 0.
        PolledTile pa, pb;
        pa.issue(a.LP + (int64_t)tail_tile_id(a.nb, c, 0) * (NB * NB));
        pb.issue(a.LP + (int64_t)tail_tile_id(a.nb, c - 1, 0) * (NB * NB));
        double a2l[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
#pragma unroll 1
        for (int s = 0; s < c - 2; ++s) {
            double* const opA = lds + ((c - 2 - s) & 1) * (2 * NB * PS);
            double* const opB = opA + NB * PS;
            pa.finish(a.LP + (int64_t)tail_tile_id(a.nb, c, s) * (NB * NB), x.spin_limit, x.info);
            pa.store(opA);
            pb.finish(a.LP + (int64_t)tail_tile_id(a.nb, c - 1, s) * (NB * NB), x.spin_limit, x.info);
            pb.store(opB);
            pa.issue(a.LP + (int64_t)tail_tile_id(a.nb, c, s + 1) * (NB * NB));
            pb.issue(a.LP + (int64_t)tail_tile_id(a.nb, c - 1, s + 1) * (NB * NB));
            __syncthreads(); // this step's operands are in LDS (and every wave is through with the pair of step s-1)
            mm64<false>(opA, opB, wm, wn, lane, a2l);
            syrk40<NB>(opA, 0, wave, lane, a2v);
        }
        // The last step, s = c-2.  BOTH of its tiles are late: L(c-1, c-2) is what the chain workgroup before this one has only just
        // solved, L(c, c-2) what the tile below it has — each published in two halves, columns 0..31 behind phase A of its solve,
        // 32..63 behind phase B some 3 us later.  Each half's products as it comes (k = 0..31, then 32..63: the order of the whole
        // product), this workgroup's own words watched without a pause: 1.4 us of matrix-core time behind the second halves
        // instead of 2.8.
        double* const opA = lds;
        double* const opB = lds + NB * PS;
        {
            const int i = threadIdx.x & 63, kk0 = threadIdx.x >> 6;
            const unsigned long long* ga = reinterpret_cast<const unsigned long long*>(a.LP + (int64_t)tail_tile_id(a.nb, c, c - 2) * (NB * NB)) + i + kk0 * NB;
            const unsigned long long* gb = reinterpret_cast<const unsigned long long*>(a.LP + (int64_t)tail_tile_id(a.nb, c - 1, c - 2) * (NB * NB)) + i + kk0 * NB;
            unsigned long long ha[4] = {pa.b[0], pa.b[1], pa.b[2], pa.b[3]}, hb[4] = {pb.b[0], pb.b[1], pb.b[2], pb.b[3]};
            chain_watch2(ga, ha, gb, hb, x.spin_limit, x.info);
            TTS2(x, true, 8);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                opA[(kk0 + 8 * q) * PS + i] = __longlong_as_double((long long)ha[q]);
                opB[(kk0 + 8 * q) * PS + i] = __longlong_as_double((long long)hb[q]);
            }
            __syncthreads(); // columns 0..31 of both tiles in LDS; every wave is through with pair 1
#pragma unroll
            for (int it = 0; it < 8; ++it)
                T[(ccol + 2 * it) * PS + crow] = cl[it];
            mmk<false, 32, 4>(opA, 0, opB, 0, wm, wn, lane, a2l);
            syrk40<32>(opA, 0, wave, lane, a2v);
            unsigned long long ka[4] = {pa.b[4], pa.b[5], pa.b[6], pa.b[7]}, kb[4] = {pb.b[4], pb.b[5], pb.b[6], pb.b[7]};
            chain_watch2(ga + 32 * NB, ka, gb + 32 * NB, kb, x.spin_limit, x.info);
            TTS2(x, true, 9);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                opA[(32 + kk0 + 8 * q) * PS + i] = __longlong_as_double((long long)ka[q]);
                opB[(32 + kk0 + 8 * q) * PS + i] = __longlong_as_double((long long)kb[q]);
            }
            __syncthreads(); // columns 32..63 (and T)
            TTS2(x, true, 10);
            mmk<false, 32, 4>(opA, 32, opB, 32, wm, wn, lane, a2l);
            syrk40<32>(opA, 32, wave, lane, a2v);
#pragma unroll
            for (int q = 0; q < 4; ++q) // first look at X11 / L21 of block c-1, device scope: in steady state they have just become
                                        // visible, and the load's way passes under the products' tail and the update of T below
                xb[q] = __hip_atomic_load(Sp + 512 * q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // T -= all the loop's products, in place: a lane's own elements
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                double* t = T + (wn + 4 * n + dcol) * PS + wm + 16 * m + drow;
                *t = *t - a2l[m][n];
            }
    }
    else {
#pragma unroll
        for (int it = 0; it < 8; ++it)
            T[(ccol + 2 * it) * PS + crow] = cl[it];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            xb[q] = __hip_atomic_load(Sp + 512 * q, __ATOMIC_RELAXED, POLL_FIRST_SCOPE);
    }
    TTS(c, 0);
    // ---- phase A: X11 and L21 of block c-1, polled value by value (diag_flow.h: DiagEarly) ----
    {
        chain_watch<4>(Sp, xb, x.spin_limit, x.info);
        TTS2(x, true, 0);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int e = threadIdx.x + 512 * q; // X11: e = k + 32 c ; L21: e = c + 32 k
            X11[(e >> 5) * 34 + (e & 31)] = __longlong_as_double((long long)xb[q]);
            Ld[(e & 31) * 34 + (e >> 5)] = __longlong_as_double((long long)xb[2 + q]); // Ld[c][k] = L21[c][k]
        }
    }
    __syncthreads(); // (A1) T, X11, L21 in LDS; pair 0 is free
    diag_flow_init(reinterpret_cast<DiagSync*>(lds + CH_AUX + DIAG_LTB + NB));
    double y1[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    tri_solve32(T, 0, X11, wm, hn, lane, y1); // Y1 = T1 X11^T
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
            Ys[(hn + 4 * n + dcol) * PS + wm + 16 * m + drow] = y1[m][n];
    __syncthreads(); // (A2) Y1 in Ys; every wave is through with T[:, 0:32]
    TTS2(x, true, 6);
    double u[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    mmk<true, 32, 2, 34>(Ys, 0, Ld, 0, wm, hn, lane, u); // Y1 L21^T
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            double* t = T + (32 + hn + 4 * n + dcol) * PS + wm + 16 * m + drow; // (a lane's own elements)
            *t = *t - u[m][n];
            T[(hn + 4 * n + dcol) * PS + wm + 16 * m + drow] = y1[m][n]; // the first half of L(c, c-1), for the matrix
        }
    { // columns 0..31 of L(c, c-1) are final: the polled copy starts its way now
        const int i = threadIdx.x & 63, kk0 = threadIdx.x >> 6;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int col = kk0 + 8 * q;
            __hip_atomic_store(pub + i + NB * col, Ys[col * PS + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    TTS2(x, true, 7);
    // first look at X22 (in steady state it arrives about now: the load's way passes under the product)
    unsigned long long xc[2];
    xc[0] = __hip_atomic_load(Sp + 2048, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    xc[1] = __hip_atomic_load(Sp + 2048 + 512, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    syrk40<32>(Ys, 0, wave, lane, a2v); // + Y1 Y1^T
    TTS2(x, true, 1);
    // ---- phase B: X22 ----
    {
        chain_watch<2>(Sp + 2048, xc, x.spin_limit, x.info);
        TTS2(x, true, 2);
        const int e0 = threadIdx.x, e1 = threadIdx.x + 512; // e = k + 32 c
        X22[(e0 >> 5) * 34 + (e0 & 31)] = __longlong_as_double((long long)xc[0]);
        X22[(e1 >> 5) * 34 + (e1 & 31)] = __longlong_as_double((long long)xc[1]);
    }
    __syncthreads(); // (B1) X22 in LDS, T[:, 32:64] complete, Ys free
    TTS2(x, true, 3);
    double y2[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    tri_solve32(T, 32, X22, wm, hn, lane, y2); // Y2 = T2 X22^T
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
            Ys[(hn + 4 * n + dcol) * PS + wm + 16 * m + drow] = y2[m][n];
    __syncthreads(); // (B2) Y2 in Ys; every wave is through with T[:, 32:64]
    TTS2(x, true, 4);
    syrk40<32>(Ys, 0, wave, lane, a2v);    // + Y2 Y2^T
    syrk40_store_neg(Dl, wave, lane, a2v); // the diagonal block's lower triangle, where the factorisation reads it
    // (off the chain: the other 32 columns of L(c, c-1) for the tiles below — the next chain workgroup's last update step has
    // a few microseconds of slack — and for the matrix)
    {
        const int i = threadIdx.x & 63, kk0 = threadIdx.x >> 6;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int col = kk0 + 8 * q;
            __hip_atomic_store(pub + i + NB * (32 + col), Ys[col * PS + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
            T[(32 + hn + 4 * n + dcol) * PS + wm + 16 * m + drow] = y2[m][n];
    TTS2(x, true, 5);
}

// The solve of any other tile (b, c), b > c + 1: L(b, c) = tile X_c^T in the half-block form, two phases, with the chain
// workgroup's means — triangular products (tri_solve32), results through a scratch block (no write-after-read barriers: four
// barriers instead of seven), the tile's second half updated by each lane in place.  `near` (b - c <= 3: the tiles whose L the
// chain's next workgroups wait for, loop (2) above) watch their own words of the block's quarters without a pause; the others —
// hundreds in a tall launch — keep the one-word look with a pause (poll_one: their polling is memory traffic for everybody).
// own: the tile with every earlier step applied (lane = row layout).  L(b, c) is left in lds + CH_T ([kk][i]) behind a barrier.
static __device__ __forceinline__ void tail_tile_solve(const P256& x, double* __restrict__ lds, const double (&own)[8],
                                                       const double* __restrict__ Sq, double* __restrict__ pub, const bool near)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 16;
    const int hn = tri_solve_cols(wave);
    const int crow = wm + (lane & 31), ccol = wn + (lane >> 5);
    const int drow = 4 * ((lane >> 2) & 3) + (lane >> 4), dcol = lane & 3;
    double* const T = lds + CH_T;
    double* const X11 = lds + CH_X11;
    double* const Ld = lds + CH_LD;
    double* const Ys = lds + CH_YS;
    double* const X22 = lds + CH_X22;
    const unsigned long long SENT = ~0ull;
    const unsigned long long* Sp = reinterpret_cast<const unsigned long long*>(Sq) + threadIdx.x;
#pragma unroll
    for (int it = 0; it < 8; ++it)
        T[(ccol + 2 * it) * PS + crow] = own[it];
    // ---- phase A: X11 and L21 ----
    {
        unsigned long long xb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) // (first look: cacheable, see PolledTile)
            xb[q] = __hip_atomic_load(Sp + 512 * q, __ATOMIC_RELAXED, POLL_FIRST_SCOPE);
        if (near)
            chain_watch<4>(Sp, xb, x.spin_limit, x.info);
        else {
            int spins = 0;
            while (xb[0] == SENT || xb[1] == SENT || xb[2] == SENT || xb[3] == SENT) {
                if (++spins > x.spin_limit) {
                    x.info[2] = 1;
                    break;
                }
                poll_one(Sq + 1023, x.spin_limit, x.info);            // X11's last row
                poll_one(Sq + 1024 + 32 * 31, x.spin_limit, x.info);  // L21's last column
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (xb[q] == SENT)
                        xb[q] = __hip_atomic_load(Sp + 512 * q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int e = threadIdx.x + 512 * q; // X11: e = k + 32 c ; L21: e = c + 32 k
            X11[(e >> 5) * 34 + (e & 31)] = __longlong_as_double((long long)xb[q]);
            Ld[(e & 31) * 34 + (e >> 5)] = __longlong_as_double((long long)xb[2 + q]);
        }
    }
    __syncthreads(); // (A1)
    double y1[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    tri_solve32(T, 0, X11, wm, hn, lane, y1); // Y1 = T1 X11^T
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
            Ys[(hn + 4 * n + dcol) * PS + wm + 16 * m + drow] = y1[m][n];
    __syncthreads(); // (A2) Y1 in Ys; every wave is through with T[:, 0:32]
    double u[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    mmk<true, 32, 2, 34>(Ys, 0, Ld, 0, wm, hn, lane, u); // Y1 L21^T
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            double* t = T + (32 + hn + 4 * n + dcol) * PS + wm + 16 * m + drow; // (a lane's own elements)
            *t = *t - u[m][n];
            T[(hn + 4 * n + dcol) * PS + wm + 16 * m + drow] = y1[m][n];
        }
    { // columns 0..31 of L(b, c) are final: the polled copy starts its way
        const int i = threadIdx.x & 63, kk0 = threadIdx.x >> 6;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int col = kk0 + 8 * q;
            __hip_atomic_store(pub + i + NB * col, Ys[col * PS + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // ---- phase B: X22 ----
    {
        unsigned long long xc[2];
        xc[0] = __hip_atomic_load(Sp + 2048, __ATOMIC_RELAXED, POLL_FIRST_SCOPE);
        xc[1] = __hip_atomic_load(Sp + 2048 + 512, __ATOMIC_RELAXED, POLL_FIRST_SCOPE);
        if (near)
            chain_watch<2>(Sp + 2048, xc, x.spin_limit, x.info);
        else {
            int spins = 0;
            while (xc[0] == SENT || xc[1] == SENT) {
                if (++spins > x.spin_limit) {
                    x.info[2] = 1;
                    break;
                }
                poll_one(Sq + 2048 + 1023, x.spin_limit, x.info); // X22's last row
                if (xc[0] == SENT)
                    xc[0] = __hip_atomic_load(Sp + 2048, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (xc[1] == SENT)
                    xc[1] = __hip_atomic_load(Sp + 2048 + 512, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        const int e0 = threadIdx.x, e1 = threadIdx.x + 512; // e = k + 32 c
        X22[(e0 >> 5) * 34 + (e0 & 31)] = __longlong_as_double((long long)xc[0]);
        X22[(e1 >> 5) * 34 + (e1 & 31)] = __longlong_as_double((long long)xc[1]);
    }
    __syncthreads(); // (B1) X22 in LDS, T[:, 32:64] complete, Ys free
    double y2[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    tri_solve32(T, 32, X22, wm, hn, lane, y2); // Y2 = T2 X22^T
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
            Ys[(hn + 4 * n + dcol) * PS + wm + 16 * m + drow] = y2[m][n];
    __syncthreads(); // (B2) Y2 in Ys; every wave is through with T[:, 32:64]
    {
        const int i = threadIdx.x & 63, kk0 = threadIdx.x >> 6;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int col = kk0 + 8 * q;
            __hip_atomic_store(pub + i + NB * (32 + col), Ys[col * PS + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
            T[(32 + hn + 4 * n + dcol) * PS + wm + 16 * m + drow] = y2[m][n];
    __syncthreads(); // L(b, c) complete in T
}

static __device__ __forceinline__ void tail_body(const TailArgs& a, const int wgid, double* __restrict__ lds,
                                                 const KParams* __restrict__ kp = nullptr)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 16;
    const int crow = wm + (lane & 31), ccol = wn + (lane >> 5);
    int c = 0, b;
    if (a.order) {
        b = __builtin_amdgcn_readfirstlane(a.order[2 * wgid]);
        c = __builtin_amdgcn_readfirstlane(a.order[2 * wgid + 1]);
    }
    else {
        int id = wgid, colh = a.nb;
        while (id >= colh) {
            id -= colh;
            ++c;
            --colh;
        }
        b = c + id;
    }
    const int slot = tail_tile_id(a.nb, b, c); // the tile's slot in the polled buffers (independent of the dispatch order)
    const bool mute = a.spin_limit < 0;
    P256 x;
    x.A = a.A;
    x.lda = a.lda;
    x.p0 = a.t0;
    x.R0 = a.t0 + (int64_t)NB * b;
    x.Xt = a.Xt;
    x.info = a.info;
    x.mute = mute;
    x.spin_limit = mute ? -a.spin_limit : a.spin_limit;
    x.nrows = b < a.nfull ? NB : a.rhs_rows;
    x.want_d = false;
    x.Bx = lds;
    x.T0 = lds + NB * XS;
    x.T1 = x.T0 + NB * PS;
    x.T2 = x.T1 + NB * PS;
    x.S22 = a.SP;
    x.HP = a.LP;
    double* const myslot = a.LP + (int64_t)slot * (NB * NB);
    { // the other pair of buffers, for the next launch: this tile's slot (and its diagonal block's quarters)
        unsigned long long* nx = reinterpret_cast<unsigned long long*>(a.LPn + (int64_t)slot * (NB * NB));
#pragma unroll
        for (int q = 0; q < 8; ++q)
            nx[threadIdx.x + 512 * q] = ~0ull;
        if (b == c) {
            unsigned long long* ns = reinterpret_cast<unsigned long long*>(a.SPn + (int64_t)c * 3072);
#pragma unroll
            for (int q = 0; q < 6; ++q)
                ns[threadIdx.x + 512 * q] = ~0ull;
        }
    }
    if (b == c + 1 && b < a.nt)
        return; // the sub-diagonal tile (c + 1, c) belongs to the workgroup of the diagonal tile of its row (below)
    // the tile, lane = row layout
    const int crc = crow < x.nrows ? crow : x.nrows - 1;
    double cv[8];
    if (kp) {
        tail_gen_tile(a, kp, x.R0 + crc, a.t0 + (int64_t)NB * c + ccol, cv);
        if (a.Al && b >= a.nfull && threadIdx.x < NB) // the right-hand-side strip: the sweep's sentinel for these columns
            for (int p = 0; p < a.P; ++p)
                reinterpret_cast<unsigned long long*>(a.Al)[a.t0 + (int64_t)NB * c + threadIdx.x + (int64_t)p * a.ldal] = ~0ull;
    }
    else {
#pragma unroll
        for (int it = 0; it < 8; ++it)
            cv[it] = a.A[x.R0 + crc + (a.t0 + (int64_t)NB * c + ccol + 2 * it) * a.lda];
    }
    if (b == c) {
        // ---- a diagonal tile's workgroup: the chain.  It also owns the tile to the left, (c, c-1): L(c, c-1) never has to
        // travel to reach the block it completes (k_panel256's factoring strip).  Steps s < c-1 update both tiles with the same
        // polled L(c, s); step c-1 is the crossing (tail_chain_updates_and_crossing).
        double* const Dl = lds + CH_D;
        double* const Ltb = lds + CH_AUX;
        double* const invd = Ltb + DIAG_LTB;
        DiagSync* const sy = reinterpret_cast<DiagSync*>(invd + NB);
        if (c > 0) {
            double cl[8]; // tile (c, c-1)
            if (kp)
                tail_gen_tile(a, kp, x.R0 + crow, a.t0 + (int64_t)NB * (c - 1) + ccol, cl);
            else {
#pragma unroll
                for (int it = 0; it < 8; ++it)
                    cl[it] = a.A[x.R0 + crow + (a.t0 + (int64_t)NB * (c - 1) + ccol + 2 * it) * a.lda];
            }
            tail_chain_updates_and_crossing(a, x, lds, c, cl, cv);
            TTS(c, 1);
        }
        else {
#pragma unroll
            for (int it = 0; it < 8; ++it)
                Dl[crow * XS + ccol + 2 * it] = cv[it];
            diag_flow_init(sy);
        }
        __syncthreads(); // the diagonal block is complete in Dl (and nobody reads the crossing's scratch any more)
        DiagEarly ea;
        ea.mute = mute;
        ea.S = a.SP + (int64_t)c * 3072;
        TTS(c, 2);
        diag_flow(Dl, Ltb, invd, sy, a.A + x.R0 + x.R0 * a.lda, a.lda, a.Xt + (int64_t)c * (NB * NB), a.info, x.R0, wave, lane,
                  invd + NB + 8, &ea);
        TTS(c, 3);
        if (c > 0) { // L(c, c-1) into the matrix: nobody reads it there before the launch ends
            __syncthreads();
            const int i = threadIdx.x & 63, kk0 = threadIdx.x >> 6;
            double* Ag = a.A + x.R0 + (a.t0 + (int64_t)NB * (c - 1)) * a.lda;
            const double* T = lds + CH_T;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int col = kk0 + 8 * q;
                Ag[i + (int64_t)col * a.lda] = T[col * PS + i];
            }
        }
        return;
    }
    // ---- any other tile: steps 0 .. c-1, then its solve ----
    PolledTile pa, pb;
    if (c > 0) {
        pa.issue(a.LP + (int64_t)tail_tile_id(a.nb, b, 0) * (NB * NB));
        pb.issue(a.LP + (int64_t)tail_tile_id(a.nb, c, 0) * (NB * NB));
    }
    double a2[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
#pragma unroll 1
    for (int s = 0; s < c; ++s) { // (pipelined over two pairs of operand buffers, one barrier a step: see the diagonal workgroup's loop)
        double* const opA = lds + (s & 1) * (2 * NB * PS);
        double* const opB = opA + NB * PS;
        pa.finish(a.LP + (int64_t)tail_tile_id(a.nb, b, s) * (NB * NB), x.spin_limit, x.info);
        pa.store(opA);
        pb.finish(a.LP + (int64_t)tail_tile_id(a.nb, c, s) * (NB * NB), x.spin_limit, x.info);
        pb.store(opB);
        if (s + 1 < c) { // the next step's operands: on their way under this step's product
            pa.issue(a.LP + (int64_t)tail_tile_id(a.nb, b, s + 1) * (NB * NB));
            pb.issue(a.LP + (int64_t)tail_tile_id(a.nb, c, s + 1) * (NB * NB));
        }
        __syncthreads();
        mm64<false>(opA, opB, wm, wn, lane, a2);
    }
    if (c > 0) {
        double a2r[8];
        wave_tile_to_rows(a2, a2r, lane);
#pragma unroll
        for (int it = 0; it < 8; ++it)
            cv[it] -= a2r[it];
        __syncthreads(); // the operand buffers are free again
    }
    tail_tile_solve(x, lds, cv, a.SP + (int64_t)c * 3072, myslot, b - c <= 3);
    { // L(b, c) into the matrix
        const int i = threadIdx.x & 63, kk0 = threadIdx.x >> 6;
        double* Ag = a.A + x.R0 + (a.t0 + (int64_t)NB * c) * a.lda;
        const double* T = lds + CH_T;
        if (i < x.nrows) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int col = kk0 + 8 * q;
                Ag[i + (int64_t)col * a.lda] = T[col * PS + i];
            }
        }
    }
}

__global__ __launch_bounds__(512) void k_tail(TailArgs a)
{
    __shared__ __attribute__((aligned(16))) double lds[TAIL_LDS_DOUBLES]; // [Bx | T0 | T1 | T2] / [A0 | B0 | A1 | B1]: all 160 KB
    tail_body(a, (int)blockIdx.x, lds);
}
// the same generating its own tiles of K (a.Xg; the kernel parameters ride in the kernel arguments)
__global__ __launch_bounds__(512) void k_tail_g(TailArgs a, KParams kp)
{
    __shared__ __attribute__((aligned(16))) double lds[TAIL_LDS_DOUBLES];
    tail_body(a, (int)blockIdx.x, lds, &kp);
}
// G members at once: blockIdx.x = tile * G + member (the members' chains advance side by side; a wait is for a lower tile of
// the same member, i.e. a lower-numbered workgroup)
__global__ __launch_bounds__(512) void k_tail_b(TailArgs a, const BatchTab* __restrict__ bt)
{
    __shared__ __attribute__((aligned(16))) double lds[TAIL_LDS_DOUBLES];
    const int G = bt->G, gp = (int)blockIdx.x % G;
    a.A = bt_rebase(bt, gp, a.A);
    a.Xt = bt_rebase(bt, gp, a.Xt);
    a.info = bt_rebase(bt, gp, a.info);
    a.LP = bt_rebase(bt, gp, a.LP);
    a.SP = bt_rebase(bt, gp, a.SP);
    a.LPn = bt_rebase(bt, gp, a.LPn);
    a.SPn = bt_rebase(bt, gp, a.SPn);
    if (a.Xg) { // (every member's own samples, obs_mean and kernel parameters)
        a.Xg = bt_rebase(bt, gp, a.Xg);
        a.Om = bt_rebase(bt, gp, a.Om);
        a.Al = bt_rebase(bt, gp, a.Al);
    }
    tail_body(a, (int)blockIdx.x / G, lds, a.Xg ? &bt->kp[gp] : nullptr);
}

// ---- the update of a ragged order's last block, behind the data-flow launch ------------------------------------------------------
// C[0:m, 0:n] -= A[0:m, 0:k] A[0:n, 0:k]^T (lower part: i >= j) with m <= 64 rows (the ragged rows of the order + the
// right-hand-side rows), n < 64 columns and k = everything the data-flow launch factored, up to 2816: ONE tile.  Its k loop on one
// compute unit is bound by that unit's load rate — 46 us at k = 1088, 69 us at k = 1664 (profiles/r05_tail_sizes.log: N = 1700 took
// longer than N = 2048).  Here the k range is dealt to up to 32 workgroups, each leaves its partial product in a scratch slot, and
// a second launch adds the slots IN ORDER (bitwise reproducible) and subtracts the sum.
// The scratch is the pair of polled buffers the data-flow launch has just used: dead until the NEXT launch arms them again, all of
// them (tail_body: every workgroup arms its own slots of the other pair).
__global__ __launch_bounds__(256) void k_ragged_partial(const double* __restrict__ A, int64_t ld, int m, int n, int64_t k, int kc,
                                                        double* __restrict__ part)
{
    __shared__ __attribute__((aligned(16))) double As[32][NB];
    const int li = threadIdx.x & 63, lk = threadIdx.x >> 6; // loading: row li, k rows lk, lk + 4, ..
    const int ti = threadIdx.x & 15, tj = threadIdx.x >> 4; // computing: a 4 x 4 block, rows 4 ti .., columns 4 tj ..
    const int64_t k0 = (int64_t)blockIdx.x * kc, k1 = k0 + kc < k ? k0 + kc : k;
    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            acc[r][c] = 0.0;
    double nx[8]; // the next 32 k rows, on their way under this block's products
    auto fetch = [&](int64_t kb) {
#pragma unroll
        for (int q = 0; q < 8; ++q) { // (rows >= m read as zero; the B operand is the first n rows of the same strip)
            const int kk = lk + 4 * q;
            nx[q] = (kb + kk < k1 && li < m) ? A[li + (kb + kk) * ld] : 0.0;
        }
    };
    fetch(k0);
    for (int64_t kb = k0; kb < k1; kb += 32) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 8; ++q)
            As[lk + 4 * q][li] = nx[q];
        if (kb + 32 < k1)
            fetch(kb + 32);
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < 32; ++kk) {
            double a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                a[r] = As[kk][4 * ti + r];
                b[r] = As[kk][4 * tj + r];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    acc[r][c] = fma(a[r], b[c], acc[r][c]);
        }
    }
    double* out = part + (int64_t)blockIdx.x * (NB * NB);
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            out[4 * ti + r + NB * (4 * tj + c)] = acc[r][c];
}
#define RAGGED_MAX_G 32
__global__ __launch_bounds__(256) void k_ragged_fold(double* __restrict__ C, int64_t ldc, int m, int n, int G, const double* __restrict__ part)
{
    const int i = threadIdx.x & 63, j = 4 * (int)blockIdx.x + (threadIdx.x >> 6); // one element a thread, 16 workgroups
    if (i >= m || j >= n || i < j)
        return;
    // every slot's value requested before the first is added (written out to RAGGED_MAX_G: one after the other the loads cost a
    // trip to memory each — 62 us for 13 slots in one workgroup), then the sum in slot order
    double v[RAGGED_MAX_G];
#pragma unroll
    for (int g = 0; g < RAGGED_MAX_G; ++g)
        v[g] = g < G ? part[(int64_t)g * (NB * NB) + i + NB * j] : 0.0;
    double sum = 0.0;
#pragma unroll
    for (int g = 0; g < RAGGED_MAX_G; ++g)
        sum += v[g]; // (slots >= G add +0.0)
    C[i + (int64_t)j * ldc] -= sum;
}
// how the k range is dealt: G workgroups (0: not worth it / no room) of kc rows each, kc a multiple of the kernel's 32-row blocks,
// the last one not empty; also the test hook gpe_debug_ragged_split (host only)
int ragged_split(int64_t k, int64_t scratch_doubles, int* kc_out)
{
    if (k < 256 || scratch_doubles < 2 * NB * NB)
        return 0;
    int64_t G = k / 64;
    G = G > RAGGED_MAX_G ? RAGGED_MAX_G : G;
    G = G > scratch_doubles / (NB * NB) ? scratch_doubles / (NB * NB) : G;
    const int64_t kc = ((k + G - 1) / G + 31) / 32 * 32;
    G = (k + kc - 1) / kc;
    *kc_out = (int)kc;
    return (int)G;
}
// ... and the rest of a ragged order's last block in ONE more launch (round 6, later): the slots are added in order and subtracted,
// the block (jb < 64 columns, padded with the identity) is factored and inverted by diag_flow, the right-hand-side rows under it are
// solved with its inverse — what k_ragged_fold, k_diag_full and a k_gemm4 launch did one after the other with a launch gap each
// (4 + 21 + 5 us and three gaps at N = 1100: profiles/r06_ragged_orders.log).  One workgroup of 512 threads.
//   C = A[N64 .., N64 ..]: rows 0 .. jb-1 the block (lower triangle), rows jb .. jb+P-1 the right-hand-side rows; part: G slots of
//   64 x 64 (i + 64 j); Lscr: 64 x 64 doubles of scratch (diag_flow stores whole columns: into the matrix they would run over the
//   right-hand-side rows); Xt: the block's inverse, transposed, identity-padded (what the sweeps read).
__global__ __launch_bounds__(DIAG_THREADS) void k_ragged_finish(double* __restrict__ C, int64_t ldc, int jb, int P, int G,
                                                                const double* __restrict__ part, double* __restrict__ Lscr,
                                                                double* __restrict__ Xt, int* __restrict__ info, int64_t goff)
{
    __shared__ __attribute__((aligned(16))) double Ls[NB * XS];
    __shared__ __attribute__((aligned(16))) double Ltb[DIAG_LTB];
    __shared__ __attribute__((aligned(16))) double invd[NB];
    __shared__ DiagSync sy;
    __shared__ __attribute__((aligned(16))) double Xw[DIAG_XW_DOUBLES];
    __shared__ double Rr[NB * 65]; // the right-hand-side rows: Rr[p * 65 + k]
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = jb + P;
    for (int e = threadIdx.x; e < NB * 65; e += DIAG_THREADS)
        Rr[e] = 0.0;
    for (int e = threadIdx.x; e < NB * NB; e += DIAG_THREADS) // the identity the short block is padded with; zeros above the diagonal
        Ls[(e & 63) * XS + (e >> 6)] = (e & 63) == (e >> 6) ? 1.0 : 0.0;
    __syncthreads();
    // the jb live columns only (64 jb elements, i + 64 j): every slot's value of TWO elements requested before the first is added,
    // then the sums in slot order (k_ragged_fold's)
#pragma unroll 1
    for (int e0 = 0; e0 < NB * jb; e0 += 2 * DIAG_THREADS) {
        double v[2][RAGGED_MAX_G], c0[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            int e = e0 + u * DIAG_THREADS + (int)threadIdx.x;
            e = e < NB * jb ? e : NB * jb - 1;
            const int i = e & 63, j = e >> 6;
#pragma unroll
            for (int g = 0; g < RAGGED_MAX_G; ++g)
                v[u][g] = part[(int64_t)(g < G ? g : G - 1) * (NB * NB) + e];
            c0[u] = C[(i < m ? i : m - 1) + (int64_t)j * ldc];
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int e = e0 + u * DIAG_THREADS + (int)threadIdx.x;
            const int i = e & 63, j = e >> 6;
            double sum = 0.0;
#pragma unroll
            for (int g = 0; g < RAGGED_MAX_G; ++g)
                sum += g < G ? v[u][g] : 0.0;
            const double val = c0[u] - sum;
            if (e < NB * jb && i < m && i >= j) {
                if (i < jb)
                    Ls[i * XS + j] = val;
                else
                    Rr[(i - jb) * 65 + j] = val;
            }
        }
    }
    diag_flow_init(&sy);
    __syncthreads();
    diag_flow(Ls, Ltb, invd, &sy, Lscr, NB, Xt, info, goff, w, lane, Xw);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's stores of L and X^T are acknowledged
    __syncthreads();
    for (int e = threadIdx.x; e < NB * NB; e += DIAG_THREADS) {
        const int i = e & 63, j = e >> 6;
        if (i < jb && j <= i)
            C[i + (int64_t)j * ldc] = __hip_atomic_load(Lscr + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // z[p][c] = sum_k r[p][k] X[c][k]   (X^T[k + 64 c], staged through LDS: Ls is free; zero above the diagonal)
    if (P > 0) {
        for (int e = threadIdx.x; e < NB * NB; e += DIAG_THREADS)
            Ls[(e >> 6) * XS + (e & 63)] = __hip_atomic_load(Xt + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // Ls[c][k]
        __syncthreads();
        for (int e = threadIdx.x; e < P * NB; e += DIAG_THREADS) {
            const int c = e & 63, p = e >> 6;
            if (c < jb) {
                double z = 0.0;
                for (int k = 0; k <= c; ++k)
                    z = fma(Rr[p * 65 + k], Ls[c * XS + k], z);
                C[jb + p + (int64_t)c * ldc] = z;
            }
        }
    }
}
bool launch_ragged_finish(hipStream_t s, double* C, int64_t ldc, const double* A, int64_t ld, int64_t jb, int64_t P, int64_t k,
                          double* scratch, int64_t scratch_doubles, double* Xt, int* info, int64_t goff)
{
    const int64_t m = jb + P;
    if (g_batch.bt || g_batch.G != 1 || jb < 1 || jb >= NB || P < 0 || m > NB || !scratch || scratch_doubles < 3 * NB * NB)
        return false;
    int kc = 0;
    const int G = ragged_split(k, scratch_doubles - NB * NB, &kc); // (one slot is diag_flow's scratch)
    if (G < 2)
        return false;
    GPE_LAUNCH(k_ragged_partial, dim3((unsigned)G), dim3(256), 0, s, A, ld, (int)m, (int)jb, k, kc, scratch);
    GPE_LAUNCH(k_ragged_finish, dim3(1), dim3(DIAG_THREADS), 0, s, C, ldc, (int)jb, (int)P, G, (const double*)scratch,
               scratch + (int64_t)G * (NB * NB), Xt, info, goff);
    return true;
}
// false: not this shape (the caller takes the general product)
bool launch_ragged_update(hipStream_t s, double* C, int64_t ldc, const double* A, int64_t ld, int64_t m, int64_t n, int64_t k,
                          double* scratch, int64_t scratch_doubles)
{
    if (g_batch.bt || g_batch.G != 1 || m < 1 || m > NB || n < 1 || n > NB || !scratch)
        return false;
    int kc = 0;
    const int G = ragged_split(k, scratch_doubles, &kc);
    if (G < 2)
        return false;
    GPE_LAUNCH(k_ragged_partial, dim3((unsigned)G), dim3(256), 0, s, A, ld, (int)m, (int)n, k, kc, scratch);
    GPE_LAUNCH(k_ragged_fold, dim3(NB / 4), dim3(256), 0, s, C, ldc, (int)m, (int)n, G, (const double*)scratch);
    return true;
}

// ---- dispatch order of a data-flow launch ----------------------------------------------------------------------------
// Workgroups are handed out in index order and each holds a CU from its dispatch to its last store, so WHEN a tile's
// workgroup becomes resident decides whether it spends its residency working or waiting — and 256 resident workgroups are all
// there is.  Column by column (rounds 3's order) a tall launch fills the chip with the 65 - c tiles of the next four columns,
// all waiting for their column's block inverse, while the diagonal workgroup of column c + 4 — 2 (c + 3) catch-up products
// of its own — is not even dispatched: from c ~ 12 on the chain waits for catch-up work (round-4 measurement: 18.9 us per
// column in the tall launch of N = 4096 against 13 in the closing launch); in a batch of G members every member has 256 / G
// resident workgroups, i.e. no look-ahead at all.  Any order is legal in which every wait is for a lower-numbered workgroup.
// Here: time slot tau per tile (in units of columns), sorted by (tau, column, row):
//   diagonal workgroup of column c (it also owns tile (c, c-1))          as early as its operands allow: behind slot c - 2
//   tile (b, c) of the triangle, b >= c + 2                              slot max(c, b - W): just in time for row b's
//                                                                        diagonal workgroup — by then its operands are there
//   tile (b, c) below the triangle (tall launch; the right-hand-side strip)   slot c + lag: behind the chain, operands ready
// W = 0 and lag = 0: column by column.  The table is checked against the dependencies before it is used.
// the table itself, on the host: flat[2 w] = row strip, flat[2 w + 1] = tile column of workgroup w; false: a wait for a
// higher-numbered workgroup somewhere (the caller then falls back to the column-by-column order)
// Round 6: the chain workgroups come TAIL_DLEAD columns earlier than their operands allow.  Stamps of a closing launch
// (profiles/r06_closing_launch_stamps.log) show hops of 14-23 us at columns 19-28 where the chain workgroup's own catch-up
// products ("earlier updates done") end late: it was dispatched behind the tiles of column c - 2, when the 256 resident
// workgroups in front of it had retired, with 2 (c - 2) products still to do.  Dispatched four columns earlier it does most of
// them while the chain is still four columns away: N = 4096 1.127 -> 1.108 ms, 3072 0.724 -> 0.707, 2560 0.542 -> 0.532, <= 2048
// unchanged (profiles/r06_diag_lead.log; 2 ... 8 the same, 12 and 16 lose it again).  Such a workgroup may wait for a tile that
// is dispatched AFTER it — the one exception to "every wait is for a lower-numbered workgroup".  It is harmless as long as
// few of them can be in that state at once: at any point q of the dispatch order, the chain workgroups in front of q that
// wait for something at or behind q hold a CU each while everything else in front of q waits only for lower-numbered
// workgroups, i.e. makes progress on the other CUs; the table is accepted only if that number never exceeds TAIL_DLEAD_MAX_BLOCKED
// (build_tail_order checks it).  Batched launches (every member has 256 / G resident workgroups) keep the strict order.
#define TAIL_DLEAD 4
#define TAIL_DLEAD_MAX_BLOCKED 16
static bool build_tail_order(int nt, int nb, int W, int lag, std::vector<int>& flat, int dlead = 0)
{
    struct T {
        int key, c, b;
    };
    std::vector<T> ts;
    for (int c = 0; c < nt; ++c)
        for (int b = c; b < nb; ++b) {
            int k;
            if (b == c)
                k = 2 * c - 3 - 2 * dlead; // behind the tiles of slot c - 2 (its last operands: (c, c-2) and the diagonal workgroup c - 1)
            else if (b >= nt) // (a lag that shrinks along the launch — late columns' tiles started early for their catch-up
                              // products — measured slower at every slope: profiles/r04_lag_slope_negative.log)
                k = 2 * (c + std::max(lag, 0));
            else if (b == c + 1)
                k = 2 * c; // (owned by the diagonal workgroup of its row: this workgroup only arms its slot)
            else
                k = 2 * (W > 0 ? std::max(c, b - W) : c);
            ts.push_back(T{k, c, b});
        }
    std::stable_sort(ts.begin(), ts.end(), [](const T& x, const T& y) {
        if (x.key != y.key)
            return x.key < y.key;
        if (x.c != y.c)
            return x.c < y.c;
        return x.b < y.b;
    });
    auto tid = [&](int b, int c) { return c * nb - (c * (c - 1)) / 2 + (b - c); };
    std::vector<int> pos(ts.size());
    for (size_t i = 0; i < ts.size(); ++i)
        pos[tid(ts[i].b, ts[i].c)] = (int)i;
    // which workgroup factors diagonal block c / publishes the slot of tile (b, s)?
    auto dpos = [&](int c) { return pos[tid(c, c)]; };
    auto owner = [&](int b, int s) { return (b == s + 1 && b < nt) ? dpos(b) : pos[tid(b, s)]; };
    bool legal = true;
    std::vector<int> blocked(ts.size() + 1, 0); // difference array: chain workgroups in front of q waiting for something at / behind q
    for (const T& t : ts) {
        const int me = pos[tid(t.b, t.c)];
        if (t.b == t.c) {
            int last = -1; // the latest-dispatched workgroup this one waits for
            for (int s2 = 0; s2 < t.c - 1; ++s2)
                last = std::max(last, std::max(owner(t.c, s2), owner(t.c - 1, s2)));
            if (last > me) {
                if (dlead <= 0)
                    legal = false;
                ++blocked[(size_t)me + 1]; // counts at q = me + 1 .. last
                --blocked[(size_t)last + 1];
            }
            if (t.c > 0)
                legal = legal && dpos(t.c - 1) < me;
        }
        else if (!(t.b == t.c + 1 && t.b < nt)) {
            for (int s2 = 0; s2 < t.c && legal; ++s2)
                legal = owner(t.b, s2) < me && owner(t.c, s2) < me;
            legal = legal && dpos(t.c) < me;
        }
        if (!legal)
            break;
    }
    for (size_t q = 1, run = 0; q < blocked.size() && legal; ++q) {
        run += blocked[q];
        legal = (int)run <= TAIL_DLEAD_MAX_BLOCKED;
    }
    flat.assign(2 * ts.size(), 0);
    for (size_t i = 0; i < ts.size(); ++i) {
        flat[2 * i] = ts[i].b;
        flat[2 * i + 1] = ts[i].c;
    }
    return legal;
}
static const int* tail_order(int nt, int nb, int dlead, int lag)
{
    const int W = 0; // (the just-in-time window of the table: measured as a loss — kept in build_tail_order for the record)
    if (dlead <= 0 && lag <= 0)
        return nullptr;
    static std::mutex mu;
    static std::map<std::array<int, 6>, int*> cache;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const std::array<int, 6> key{dev, nt, nb, dlead, lag, 0};
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(key);
    if (it != cache.end())
        return it->second;
    std::vector<int> flat;
    int* d = nullptr;
    if (build_tail_order(nt, nb, W, lag, flat, dlead) || (dlead > 0 && build_tail_order(nt, nb, W, lag, flat, 0))) {
        if (hipMalloc(&d, sizeof(int) * flat.size()) != hipSuccess || hipMemcpy(d, flat.data(), sizeof(int) * flat.size(), hipMemcpyHostToDevice) != hipSuccess)
            d = nullptr;
    }
    else
        fprintf(stderr, "gpe: tail_order(%d, %d, lead %d, lag %d) violates a dependency — column-by-column order used\n", nt, nb, dlead, lag);
    cache[key] = d;
    return d;
}
// test hook: the work split of the chain workgroup's products (syrk40 / tri_solve32) as the device code has it
void debug_chain_split(int wave, int* units10, int* cols)
{
    for (int q = 0; q < 5; ++q)
        syrk40_units(wave, q, units10[2 * q], units10[2 * q + 1]);
    *cols = tri_solve_cols(wave);
}
// test hook (include/gpe.h: gpe_debug_tail_order): 1 if the dispatch table of a data-flow launch of nt tile columns x nb row
// strips is a permutation of its tiles in which every wait is for a lower-numbered workgroup, 0 if not; host only
int debug_tail_order(int nt, int nb, int lag, int pair)
{
    if (pair)
        return -1; // (the two-blocks-per-chain-workgroup form of round 4 was removed in round 6)
    if (nt < 1 || nb < nt || nb > 4096)
        return -1;
    std::vector<int> flat;
    if (!build_tail_order(nt, nb, 0, lag, flat, 0)) // the strict table (batched launches)
        return 0;
    if (!build_tail_order(nt, nb, 0, lag, flat, TAIL_DLEAD)) // ... and the one single launches use (checked below)
        return 0;
    std::vector<char> seen((size_t)nt * nb, 0);
    size_t n = 0;
    for (size_t i = 0; i + 1 < flat.size(); i += 2) {
        const int b = flat[i], c = flat[i + 1];
        if (c < 0 || c >= nt || b < c || b >= nb || seen[(size_t)c * nb + b])
            return 0;
        seen[(size_t)c * nb + b] = 1;
        ++n;
    }
    return n == (size_t)(nt * nb - nt * (nt - 1) / 2) ? 1 : 0;
}

// Tile columns t0 .. t1-1 (whole 64-blocks) of the rows t0 .. M-1: N64 - t0 full row strips (N64 = the matrix order rounded down
// to 64; t1 == N64: the closing launch) and, as one more row strip, the M - N64 <= 64 rows below them — right-hand-side rows and
// the rows of a ragged last block the caller finishes.  Fully updated by everything in front of t0.  buf_cur / buf_next:
// tail_buf_doubles(nt, nb) each, all-ones (this launch arms buf_next).  gen: the launch generates its tiles of K — only ever
// given with t0 = 0 and t1 = N64, the launch that is the whole factorisation; what k_tail_g carries for a tall launch
// (t1 < N64) is no longer reached and leaves with the next change to that kernel
void launch_tail(hipStream_t s, double* A, int64_t lda, int64_t t0, int64_t t1, int64_t N64, int64_t M, double* Xt_all, int* info,
                 double* buf_cur, double* buf_next, const TailGen* gen)
{
    TailArgs a{};
    a.A = A;
    a.lda = lda;
    a.t0 = t0;
    a.nt = (int)((t1 - t0) / NB);
    a.nfull = (int)((N64 - t0) / NB);
    a.rhs_rows = (int)(M - N64);
    a.nb = a.nfull + (a.rhs_rows > 0 ? 1 : 0);
    a.Xt = Xt_all + (t0 / NB) * (NB * NB);
    a.info = info;
    a.SP = buf_cur;
    a.LP = buf_cur + (int64_t)a.nt * 3072;
    a.SPn = buf_next;
    a.LPn = buf_next + (int64_t)a.nt * 3072;
    a.spin_limit = flow_spin_limit();
    // measured (profiles/r04_dispatch_order.log, N = 4096): lag 2..4 -> 794-800 evaluations/s against 735 column by column; a
    // just-in-time window W > 0 LOSES (6: 675, 8: 694, 12: 738, 16: 770): a tile dispatched late has its catch-up products still
    // to do when its row's diagonal workgroup asks for it; waiting workgroups are not what limits the closing launch
    a.order = tail_order(a.nt, a.nb, g_batch.bt ? 0 : TAIL_DLEAD, /* lag */ 3);
    const int64_t tiles = tail_tiles(a.nt, a.nb);
    if (gen) {
        a.Xg = gen->Xg;
        a.ldx = gen->ldx;
        a.Ns = gen->Ns;
        a.Om = gen->Om;
        a.ldom = gen->ldom;
        a.Al = gen->Al;
        a.ldal = gen->ldal;
        a.P = gen->P;
    }
    FlowGate gate(s); // (one data-flow launch at a time on the device: dev.h)
    if (g_batch.bt)
        GPE_LAUNCH(k_tail_b, dim3((unsigned)(tiles * g_batch.G)), dim3(512), 0, s, a, g_batch.bt);
    else if (gen)
        GPE_LAUNCH(k_tail_g, dim3((unsigned)tiles), dim3(512), 0, s, a, *gen->kp);
    else
        GPE_LAUNCH(k_tail, dim3((unsigned)tiles), dim3(512), 0, s, a);
}

#ifdef DIAG_TIMING
void dump_tail_timing(int nt)
{
    long long h[64][4];
    hipMemcpyFromSymbol(h, HIP_SYMBOL(g_tail_ts), sizeof(h));
    const long long t0 = h[0][2];
    printf("k_tail, the diagonal workgroups (us after the first one starts factoring): column | earlier updates done | its left tile solved, block complete | factoring | panel wave done\n");
    for (int c = 0; c < nt && c < 64; ++c)
        printf("  %2d | %7.2f | %7.2f | %7.2f | %7.2f   (step %5.2f)\n", c, c ? (h[c][0] - t0) * 0.01 : 0.0, c ? (h[c][1] - t0) * 0.01 : 0.0,
               (h[c][2] - t0) * 0.01, (h[c][3] - t0) * 0.01, c ? (h[c][2] - h[c - 1][2]) * 0.01 : 0.0);
    long long cy[64][4];
    hipMemcpyFromSymbol(cy, HIP_SYMBOL(g_tail_cyc), sizeof(cy));
    printf("  factoring -> panel wave done, per column: us | shader-clock cycles | MHz\n   ");
    for (int c = 0; c < nt && c < 64; ++c)
        printf(" %d: %.2f %lld %.0f |", c, (h[c][3] - h[c][2]) * 0.01, cy[c][3] - cy[c][2], (cy[c][3] - cy[c][2]) / ((h[c][3] - h[c][2]) * 0.01));
    printf("\n");
    long long g[64][12];
    hipMemcpyFromSymbol(g, HIP_SYMBOL(g_tail_ts2), sizeof(g));
    printf("  between two blocks, us after the panel wave of column c-1 is through: X11/L21 seen | phase A done | X22 seen | X22 in LDS | Y2 written | second half product done | block complete | factoring\n");
    for (int c = 1; c < nt && c < 64; ++c) {
        const long long p = h[c - 1][3];
        printf("  %2d | %6.2f | %6.2f | %6.2f | %6.2f | %6.2f | %6.2f | %6.2f | %6.2f   (updates done %6.2f; inside phase A: Y1 in LDS %6.2f, T2 updated + first half out %6.2f)\n", c, (g[c][0] - p) * 0.01, (g[c][1] - p) * 0.01, (g[c][2] - p) * 0.01,
               (g[c][3] - p) * 0.01, (g[c][4] - p) * 0.01, (g[c][5] - p) * 0.01, (h[c][1] - p) * 0.01, (h[c][2] - p) * 0.01, (h[c][0] - p) * 0.01,
               (g[c][6] - p) * 0.01, (g[c][7] - p) * 0.01);
        if (c >= 2)
            printf("       the last update step: first halves of L(c, c-2), L(c-1, c-2) seen %6.2f | second halves seen %6.2f | in LDS %6.2f\n",
                   (g[c][8] - p) * 0.01, (g[c][9] - p) * 0.01, (g[c][10] - p) * 0.01);
    }
}
#endif
