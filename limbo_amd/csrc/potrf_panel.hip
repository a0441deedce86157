// potrf_panel.hip — the panel launches of the blocked Cholesky (gfx950), each described where it is defined: k_diag(_b),
// k_panel_step(_b) with k_head_copy, k_panel256, k_upd_fused.
#include "potrf_tile.h"
#ifdef DIAG_TIMING
__device__ long long g_diag_ts[32]; // k_diag (diag_body): start | block in LDS | factored and inverted
__device__ long long g_panel_ts[64];
#define PTS(i) do { if (threadIdx.x == 0 && (blockIdx.x == 0 || blockIdx.x == gridDim.x - 1)) g_panel_ts[(blockIdx.x == 0 ? 0 : 32) + (i)] = clock64(); } while (0)
__device__ long long g_p256_ts[5][32]; // k_panel256: strips 0..3 and the last one; [6 S + i] = stamp i of step S, [30] start, [31] end
#define P2TS(i) do { if (threadIdx.x == 0 && (blockIdx.x < 4 || blockIdx.x == gridDim.x - 1)) g_p256_ts[blockIdx.x < 4 ? blockIdx.x : 4][(i)] = wall_clock64(); } while (0)
#else
#define PTS(i) do { } while (0)
#define P2TS(i) do { } while (0)
#endif
#if defined(DIAG_TIMING) && !defined(DIAG_NO_STAMPS) // (DIAG_NO_STAMPS: the array exists for tools/diagbench.hip, the kernel is the shipped one)
#define TS(i) do { if (threadIdx.x == 0) g_diag_ts[i] = clock64(); } while (0)
#else
#define TS(i) do { } while (0)
#endif

// The block the fused panel steps start from: L11 in place and X^T = L11^-T into Xt (the quarter above the
// diagonal stays zero), by the data-flow form of diag_flow.h.  Full 64 x 64 blocks only.  It is in this file, not with
// k_diag_full: its instructions depend on which other callers of diag_flow share the file (profiles/potrf_split_identity.txt).
static __device__ __forceinline__ void diag_body(double* __restrict__ A, int64_t lda, double* __restrict__ Xt,
                                                 int* __restrict__ info, int64_t goff)
{
    __shared__ __attribute__((aligned(16))) double Ls[NB * XS];
    __shared__ __attribute__((aligned(16))) double Ltb[DIAG_LTB];
    __shared__ __attribute__((aligned(16))) double invd[NB];
    const int r = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    __shared__ DiagSync sy;
    __shared__ __attribute__((aligned(16))) double Xw[DIAG_XW_DOUBLES];
    static_assert(DIAG_H_DOUBLES <= DIAG_LTB, "H fits where the round buffers were");
    TS(0);
    for (int e = threadIdx.x; e < NB * NB; e += DIAG_THREADS)
        Ls[(e & 63) * XS + (e >> 6)] = A[(e & 63) + (int64_t)(e >> 6) * lda];
    diag_flow_init(&sy);
    __syncthreads();
    TS(1);
    diag_flow(Ls, Ltb, invd, &sy, A, lda, Xt, info, goff, w, r, Xw);
    TS(2);
    return;
}
// entry points: single GP (the round-1 kernel, unchanged) / batched (gridDim.z GPs, pointers rebased; dev.h)
__global__ __launch_bounds__(DIAG_THREADS) void k_diag(double* __restrict__ A, int64_t lda, double* __restrict__ Xt,
                                              int* __restrict__ info, int64_t goff)
{
    diag_body(A, lda, Xt, info, goff);
}
__global__ __launch_bounds__(DIAG_THREADS) void k_diag_b(double* __restrict__ A, int64_t lda, double* __restrict__ Xt,
                                                int* __restrict__ info, int64_t goff, const BatchTab* __restrict__ bt)
{
    BT_REBASE(bt, A);
    BT_REBASE(bt, Xt);
    BT_REBASE(bt, info);
    diag_body(A, lda, Xt, info, goff);
}

// ---------------------------------------------------------------------------------------------
// k_panel_step — one 64-column step of the blocked factorisation below an already factored
// diagonal block, fused into ONE launch (a dependent launch costs ~3.4 us here, so the
// three-launch form [L21 = A21 X^T | in-panel update | next k_diag] pays 10 us of floor per step):
//   workgroup b owns rows R_b = [r0 + 64 b, +64) of the panel (r0 = j0 + 64):
//     1. L_b = A[R_b, j0:j0+64] X^T                                    (matrix cores, X = L11^-1)
//     2. for every remaining 64-column block t of the outer panel with t <= b:
//          A[R_b, block t] -= L_b L_t^T,  L_t = rows of block t of the same product.
//        L_t belongs to another workgroup; instead of an inter-workgroup hand-off it is recomputed
//        here (256 MFMAs per wave, hidden behind workgroup 0's serial diagonal factorisation).
//     3. workgroup 0 then holds the fully updated next diagonal block and factors + inverts it
//        (same code as k_diag), so the next step needs no separate diagonal launch.
// Requires full 64-column blocks (host falls back to the three-launch form otherwise).
// ---------------------------------------------------------------------------------------------

// The same solve with ALL of X = L11^-1 (lower triangular; diag_flow.h leaves the off-diagonal quarter too): ONE product,
// Y[i][c] = sum_{k <= c} T[i][k] X[c][k], two barriers instead of six.  A wave's 16 columns need k < wn + 16 only.
static __device__ __forceinline__ void trsm_tile_full(double* __restrict__ T, const double* __restrict__ Bx, int lane, int wave)
{
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 16;
    const int drow = 4 * ((lane >> 2) & 3) + (lane >> 4), dcol = lane & 3;
    double y[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
            y[m][n] = 0.0;
    switch (wave >> 1) {
    case 0: mmk<true, 16, 4>(T, 0, Bx, 0, wm, wn, lane, y); break;
    case 1: mmk<true, 32, 4>(T, 0, Bx, 0, wm, wn, lane, y); break;
    case 2: mmk<true, 48, 4>(T, 0, Bx, 0, wm, wn, lane, y); break;
    default: mmk<true, 64, 4>(T, 0, Bx, 0, wm, wn, lane, y); break;
    }
    __syncthreads(); // every wave has read what it needs of T
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
            T[(wn + 4 * n + dcol) * PS + wm + 16 * m + drow] = y[m][n];
    __syncthreads();
}

// 64 x 64 tile of column-major G (rows clamped to nrows) <-> registers <-> T[kk * PS + i]; 512 threads
struct TileRegs {
    double v[8];
    __device__ __forceinline__ void load(const double* __restrict__ G, int64_t ld, int nrows)
    {
        const int i = threadIdx.x & 63, kk0 = threadIdx.x >> 6;
        const int ic = i < nrows ? i : nrows - 1;
#pragma unroll
        for (int q = 0; q < 8; ++q)
            v[q] = G[ic + (int64_t)(kk0 + 8 * q) * ld];
    }
    // the same tile (ld = 64) straight from device-coherent memory: written by another workgroup of THIS launch with
    // write-through stores (panel_step_body, head-tile hand-over), possibly on another XCD behind another L2
    __device__ __forceinline__ void load_coherent(const double* G)
    {
        const int i = threadIdx.x & 63, kk0 = threadIdx.x >> 6;
#pragma unroll
        for (int q = 0; q < 8; ++q)
            v[q] = __hip_atomic_load(G + i + (int64_t)(kk0 + 8 * q) * NB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void store(double* __restrict__ T) const
    {
        const int i = threadIdx.x & 63, kk0 = threadIdx.x >> 6;
#pragma unroll
        for (int q = 0; q < 8; ++q)
            T[(kk0 + 8 * q) * PS + i] = v[q];
    }
};

#define PANEL_PRE 3 // head tiles held in registers (nbo = 256 needs 3)

// dnext >= 0: the workgroup that owns rows dnext .. dnext+63 (the next OUTER panel's first diagonal block) also
// adds its L L^T to the 64 x 64 scratch Dacc (lane = row order of a workgroup's C tile; dinit: starts the sum) —
// and, when dfirst >= 0, the same product of the column block at dfirst (the panel's first, whose own step has
// no workgroup to spare; done in the step where that workgroup has the most slack).  k_upd_fused subtracts the
// sum from the block and only has to factor it.  (Not subtracted from A directly: the second stream's GEMMs
// may still be updating that block.)
static __device__ __forceinline__ void panel_step_body(double* __restrict__ A, int64_t lda, int64_t j0, int64_t M, int nt,
                                                       const double* __restrict__ Xt_cur, double* __restrict__ Xt_next,
                                                       int do_next, int* __restrict__ info, double* __restrict__ Hs,
                                                       int64_t dnext, int64_t dfirst, int dinit, double* __restrict__ Dacc,
                                                       gpe_epoch_t* hflag, gpe_epoch_t epoch, int spin_limit, const int bx)
{
    // one LDS array, carved: [Bx | T0 | T1]; workgroup 0 re-carves it as [Ls | Ltb | invd | sync | Xw]
    __shared__ __attribute__((aligned(16))) double lds[NB * XS + 2 * NB * PS];
    static_assert(NB * XS + DIAG_LTB + NB + 8 + DIAG_XW_DOUBLES <= NB * XS + 2 * NB * PS, "workgroup 0's carve fits");
    double* Bx = lds;
    double* T0 = lds + NB * XS;
    double* T1 = T0 + NB * PS;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 16;
    const int b = bx;
    const int64_t r0 = j0 + NB, R0 = r0 + (int64_t)NB * b;
    const int nrows = (int)((M - R0 < NB) ? M - R0 : NB);
    const int tmax = (b < nt - 1) ? b : nt - 1;

    // every global load this workgroup needs before its first product goes out now: X, its own
    // tile, and the head tiles it will re-derive (one exposed memory latency instead of one per tile)
    PTS(0);
    TileRegs own, head[PANEL_PRE];
    own.load(A + R0 + j0 * lda, lda, nrows);
    double xv[8];
#pragma unroll
    for (int q = 0; q < 8; ++q)
        xv[q] = Xt_cur[threadIdx.x + 512 * q];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int e = threadIdx.x + 512 * q;
        Bx[(e >> 6) * XS + (e & 63)] = xv[q]; // Bx[c][k] = X[c][k]
    }
    own.store(T0);
    // the C tile of the first update (for workgroup 0: the next diagonal block) is fetched now, under
    // the triangular solve, instead of at the top of the update loop
    // C tiles travel in the lane = row layout (wave_tile_to_rows): element it of a thread is
    // row wm + (lane & 31), column wn + 2 it + (lane >> 5) of the 64 x 64 tile
    const int crow = wm + (lane & 31), ccol = wn + (lane >> 5);
    const int crc = crow < nrows ? crow : nrows - 1;
    double c0v[8];
    if (tmax >= 0) {
#pragma unroll
        for (int it = 0; it < 8; ++it)
            c0v[it] = A[R0 + crc + (r0 + ccol + 2 * it) * lda];
    }
    __syncthreads();
    PTS(1);

    // 1. L_b = A_b L11^-T  (half-block form of the inverse, in place in T0)
    trsm_tile_full(T0, Bx, lane, wave);
    PTS(2);
    {
        // Row blocks b < nt are the "head" tiles other workgroups re-derive from A while this one
        // runs: they must not be overwritten in place here.  Their L goes to the scratch tile Hs[b]
        // and k_head_copy moves it into A after the panel's fused steps.
        const int i = threadIdx.x & 63, kk0 = threadIdx.x >> 6;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int col = kk0 + 8 * q;
            const double v = T0[col * PS + i];
            if (b < nt) { // write-through: other XCDs read this tile during this launch (the hand-over)
                __hip_atomic_store(Hs + (int64_t)b * (NB * NB) + i + NB * col, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                // with the hand-over nobody re-derives anything from A's head rows: L goes into place as well and the
                // panel needs no k_head_copy behind it (a launch in front of every look-ahead update)
                if (hflag)
                    A[R0 + i + (j0 + col) * lda] = v;
            }
            else if (i < nrows)
                A[R0 + i + (j0 + col) * lda] = v;
        }
    }

    PTS(3);
    // Head tiles change hands instead of being re-derived by every workgroup (round 2; the stamps of tools/kbench_t showed
    // the last workgroup of a first step at 66 k cycles, 47 k of them three re-derived head tiles + updates, against 40 k for
    // workgroup 0 INCLUDING the diagonal block).  A head workgroup publishes: its tile is in Hs, device-wide, then
    // hflag[b] = this launch's epoch (a value no earlier launch used: the words are never reset).  Consumers need only
    // lower-numbered head tiles and the heads wait for nobody but lower-numbered heads, so with workgroups dispatched in
    // index order nobody can wait for a workgroup that is not running; the wait is bounded all the same (below).
    const bool mute = spin_limit < 0; // test hook (GPE_HANDOVER_FAULT): nobody publishes, every consumer gives up at once
    if (spin_limit < 0)
        spin_limit = -spin_limit;
    if (b < nt && hflag && !mute) {
        // The tile went out with device-scope (write-through) stores, the consumers read it and the flag with device-scope
        // loads: no release/acquire fence anywhere.  (An agent-scope release writes back the whole L2 of this XCD — every
        // dirty C tile of every workgroup on it: 7.5 k cycles when each wave issued one, 3 k for a single one, growing
        // with the number of updates in flight; tools/kbench_t.)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this thread's part of the tile is acknowledged
        __syncthreads();
        if (threadIdx.x == 0)
            __hip_atomic_store(hflag + b, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // Every wave waits for a tile's word itself (all lanes read the same word: a wave-uniform spin) and then fetches its
    // eighth of the tile: no broadcast of "it is there" through LDS, no barrier, and the three tiles' loads overlap.  (One
    // thread polling the three words in turn + two barriers + the loads took 11 k cycles from "own L written" to "tiles in
    // registers", tools/kbench_t.)  The poll is bounded; a wave that runs out of patience reports it (info[2] = 1) and the
    // host runs the evaluation again without the hand-over (engine.hip, compute_finish) — its tile may be garbage by then.
    const bool handed = hflag != nullptr; // nullptr: no hand-over in this launch (GPE_PANEL_HANDOVER=0): re-derive
    gpe_epoch_t seen[PANEL_PRE];
#pragma unroll
    for (int t = 0; t < PANEL_PRE; ++t) // all words at once: a poll is a round trip to memory even when the word is set
        seen[t] = (handed && t <= tmax && t != b) ? __hip_atomic_load(hflag + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : epoch;
#pragma unroll
    for (int t = 0; t < PANEL_PRE; ++t)
        if (t <= tmax && t != b) {
            if (handed) {
                int spins = 0;
                while (seen[t] != epoch) {
                    if (++spins > spin_limit) {
                        if (lane == 0)
                            info[2] = 1;
                        break;
                    }
                    seen[t] = __hip_atomic_load(hflag + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                // the tile's loads may not be moved above the poll by the compiler (the hardware returns a wave's
                // loads in order; relaxed atomics alone do not order them in the language): a zero-cost fence
                asm volatile("" ::: "memory");
                head[t].load_coherent(Hs + (int64_t)t * (NB * NB));
            }
            else
                head[t].load(A + r0 + (int64_t)NB * t + j0 * lda, lda, NB);
        }
    // 2. in-panel updates of this row block
    double cres[8]; // workgroup 0: the updated next diagonal block (lane = row layout)
#pragma unroll 1
    for (int t = 0; t <= tmax; ++t) {
        double* Cg = A + R0 + (r0 + (int64_t)NB * t) * lda;
        double cv[8];
#pragma unroll
        for (int it = 0; it < 8; ++it)
            cv[it] = (t == 0) ? c0v[it] : Cg[crc + (int64_t)(ccol + 2 * it) * lda];
        const double* Bop = T0;
        if (t == 0)
            PTS(10);
        if (t != b) { // head tile of another row block: recompute L_t = A_t X^T
            if (t == 0)
                head[0].store(T1);
            else if (t == 1)
                head[1].store(T1);
            else if (t == 2)
                head[2].store(T1);
            else {
                TileRegs late;
                if (handed) {
                    int spins = 0;
                    while (__hip_atomic_load(hflag + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch)
                        if (++spins > spin_limit) {
                            if (lane == 0)
                                info[2] = 1;
                            break;
                        }
                    asm volatile("" ::: "memory"); // as above: the tile's loads stay behind the poll
                    late.load_coherent(Hs + (int64_t)t * (NB * NB));
                }
                else
                    late.load(A + r0 + (int64_t)NB * t + j0 * lda, lda, NB);
                late.store(T1);
            }
            __syncthreads();
            if (!handed) {
                trsm_tile_full(T1, Bx, lane, wave);
            }
            Bop = T1;
        }
        double a2[2][4];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n)
                a2[m][n] = 0.0;
        if (t == 0)
            PTS(11);
        mm64<false>(T0, Bop, wm, wn, lane, a2);
        if (t == 0)
            PTS(12);
        double a2r[8];
        wave_tile_to_rows(a2, a2r, lane);
        if (t == 0)
            PTS(13);
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const double v = cv[it] - a2r[it];
            if (t == 0)
                cres[it] = v;
            // workgroup 0 factors this tile next and writes L over it: no need to store the update
            if (crow < nrows && !(b == 0 && do_next))
                Cg[crow + (int64_t)(ccol + 2 * it) * lda] = v;
        }
        if (t == 0)
            PTS(14);
        __syncthreads(); // T1 is free again
        if (t == 0)
            PTS(15);
    }

    // 2b. the piece(s) of the next outer panel's first diagonal block that this workgroup can provide
    if (dnext >= 0 && R0 == dnext) {
        double pr[2][4];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n)
                pr[m][n] = 0.0;
        double cd[8];
        if (!dinit) { // a later step of the panel: add to the running sum
#pragma unroll
            for (int it = 0; it < 8; ++it)
                cd[it] = Dacc[threadIdx.x + 512 * it];
        }
        mm64<false>(T0, T0, wm, wn, lane, pr); // own L (this step's column block) times its transpose
        if (dfirst >= 0) {                      // and the same rows of the column block at dfirst
            TileRegs lf;
            lf.load(A + dnext + dfirst * lda, lda, NB);
            __syncthreads(); // T1's last readers (head-tile products) are done
            lf.store(T1);
            __syncthreads();
            mm64<false>(T1, T1, wm, wn, lane, pr);
        }
        double prr[8];
        wave_tile_to_rows(pr, prr, lane);
#pragma unroll
        for (int it = 0; it < 8; ++it)
            Dacc[threadIdx.x + 512 * it] = (dinit ? 0.0 : cd[it]) + prr[it];
    }

    PTS(4);
    // 3. workgroup 0: factor the next diagonal block (block t = 0 of its own rows) and invert its halves
    if (b != 0 || !do_next)
        return;
    double* Ls = lds;
    double* Ltb = Ls + NB * XS;
    double* invd = Ltb + DIAG_LTB;
#pragma unroll
    for (int it = 0; it < 8; ++it)
        Ls[crow * XS + ccol + 2 * it] = cres[it];
    {
        DiagSync* sy = reinterpret_cast<DiagSync*>(invd + NB);
        diag_flow_init(sy);
        __syncthreads();
        PTS(5);
        diag_flow(Ls, Ltb, invd, sy, A + r0 + r0 * lda, lda, Xt_next, info, r0, wave, lane, invd + NB + 8);
        PTS(6);
        return;
    }
}
// entry points: single GP (the round-1 kernel, unchanged) / batched.  Batched: blockIdx.x = b * G + gp, so that workgroup 0
// of every GP (the one that goes on to factor the next diagonal block, twice as long as the others) is dispatched first
// instead of trailing each GP's rows.
__global__ __launch_bounds__(512) void k_panel_step(double* __restrict__ A, int64_t lda, int64_t j0, int64_t M, int nt,
                                                    const double* __restrict__ Xt_cur, double* __restrict__ Xt_next,
                                                    int do_next, int* __restrict__ info, double* __restrict__ Hs,
                                                    int64_t dnext, int64_t dfirst, int dinit, double* __restrict__ Dacc,
                                                    gpe_epoch_t* hflag, gpe_epoch_t epoch, int spin_limit)
{
    panel_step_body(A, lda, j0, M, nt, Xt_cur, Xt_next, do_next, info, Hs, dnext, dfirst, dinit, Dacc, hflag, epoch, spin_limit,
                    (int)blockIdx.x);
}
__global__ __launch_bounds__(512) void k_panel_step_b(double* __restrict__ A, int64_t lda, int64_t j0, int64_t M, int nt,
                                                      const double* __restrict__ Xt_cur, double* __restrict__ Xt_next,
                                                      int do_next, int* __restrict__ info, double* __restrict__ Hs,
                                                      int64_t dnext, int64_t dfirst, int dinit, double* __restrict__ Dacc,
                                                      gpe_epoch_t* hflag, gpe_epoch_t epoch, int spin_limit,
                                                      const BatchTab* __restrict__ bt)
{
    const int G = bt->G, gp = (int)blockIdx.x % G;
    A = bt_rebase(bt, gp, A);
    Xt_cur = bt_rebase(bt, gp, Xt_cur);
    Xt_next = bt_rebase(bt, gp, Xt_next);
    info = bt_rebase(bt, gp, info);
    Hs = bt_rebase(bt, gp, Hs);
    Dacc = bt_rebase(bt, gp, Dacc);
    hflag = bt_rebase(bt, gp, hflag);
    panel_step_body(A, lda, j0, M, nt, Xt_cur, Xt_next, do_next, info, Hs, dnext, dfirst, dinit, Dacc, hflag, epoch, spin_limit,
                    (int)blockIdx.x / G);
}

// ---------------------------------------------------------------------------------------------
// k_panel256 (round 3) — ALL 64-column steps of a 256-column outer panel in ONE launch, as data flow between the
// workgroups.  The step-by-step form pays, per step, a launch boundary plus the serial sequence
//   [diagonal block | head tiles | everybody's solve | everybody's updates]
// (21 + 20 + 19 us for the three steps of a panel at N = 4096 and ~3 us between launches), although the only true chain is
//   X_s -> L(s, s) = A(s, s) X_s^T -> A(s, s+1) -= L L^T -> factor -> X_{s+1}                (~12 us per step).
// Here workgroup b owns the 64-row strip R_b = rows p0 + 64 (b + 1) .. +63 of the panel for the whole launch and keeps its
// (up to four) 64 x 64 tiles in REGISTERS between the steps: every tile is read once and written once, as L.
//   step s (column block s of the panel), strips b >= s:
//     X_s (s = 0: the diagonal block at p0 was factored by the launch before; s > 0: polled, below)  ->  L_bs = A_bs X_s^T
//     strips b <= 2 publish L_bs (a "head tile": the rows of column block b + 1)
//     A_bc -= L_bs L_{c-1,s}^T for the strip's remaining column blocks c = s+1 .. min(3, b+1)
//     strip b = s now holds the finished diagonal block of column block s + 1: it factors it (diag_flow), X_{s+1} goes out
//       quarter by quarter while it is being computed — and the strip is done.
// Nothing inside the launch is handed over with a flag: block inverses and head tiles are stored, with device-scope stores,
// into buffers that hold an all-ones pattern when the launch starts, and their consumers poll the values (P256::S22 / HP,
// PolledTile, poll_one; diag_flow.h: DiagEarly).  The launch arms the other buffer of the pair for the launch after it.
// A strip only ever waits for lower-numbered strips (X_s comes from strip s - 1 <= b - 1, head tiles from strips < b), so
// with workgroups dispatched in index order nobody waits for a workgroup that is not running (dev.h, requirement (1));
// the polls are bounded all the same and a timeout is reported exactly like k_panel_step's (info[2], the host re-runs).
// From step 1 on every strip solves in the half-block form of the inverse, in two phases (p256_half_solve): three quarters of
// the solve, and the first k-half of the factoring strip's update, run while the previous block is still being factored.
// dnext >= 0: the strip of rows dnext (the next panel's first diagonal block) also leaves sum_s L_bs L_bs^T in Dacc for
// k_upd_fused.  Full 64-column blocks, nbo = 256 only; everything else goes the step-by-step way.
// ---------------------------------------------------------------------------------------------
// head tile h = P256_H(s, t): the tile of strip t at step s (t = s..2), six per panel
#define P256_H(s, t) ((s) == 0 ? (t) : ((s) == 1 ? 2 + (t) : 5))

// (P256_POLLED_S, P256_POLLED_DOUBLES: shell_layout.h, beside the tiles that hold the two buffers)
static_assert(NB == shell::EDGE, "the shell's tiles are this file's");

// The strip that factors next solves against the block inverse in the half-block form, in two phases: three quarters of its
// solve and half of its one update run while the previous strip is still factoring (X11 and L21 of that block leave it half-way
// through, diag_flow.h: DiagEarly); what is left behind the arrival of X22 is one 64 x 32 x 32 product and the other half of the
// update.  T (64 x 64, [kk][i], stride PS) <- own L^-T; acc += (own L^-T)(own L^-T)^T over both halves of k.
// Every strip solves this way from step 1 on (PUBHALF / acc_on: the factoring strip publishes the first half of its tile after
// phase A and accumulates its update; the strip of the next panel's first diagonal block accumulates its piece of that block;
// the others only solve): what a strip still has to do once the last rows of X are out is a quarter of the solve.
// Sq: the block's polled quarters (X11 | L21 | X22, 1024 doubles each); pub (PUBHALF): where the strip's own tile goes, polled
template <int S, bool PUBHALF>
static __device__ __forceinline__ void p256_half_solve(const P256& x, double* __restrict__ T, double* __restrict__ Ld,
                                                       const double (&own)[8], double (&a2)[2][4], const bool acc_on,
                                                       const double* __restrict__ Sq, double* __restrict__ pub)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 16; // the 64 x 64 product's wave tile
    const int hn = (wave >> 1) * 8;                        // the half-block products': column within the 32-column half
    const int crow = wm + (lane & 31), ccol = wn + (lane >> 5);
    const int drow = 4 * ((lane >> 2) & 3) + (lane >> 4), dcol = lane & 3;
    double* Bx = x.Bx;
    P2TS(6 * S + 0);
#pragma unroll
    for (int it = 0; it < 8; ++it)
        T[(ccol + 2 * it) * PS + crow] = own[it];
    // ---- phase A: X11 and L21, polled value by value (diag_flow.h: DiagEarly) ----
    const unsigned long long SENT = ~0ull;
    const unsigned long long* Sp = reinterpret_cast<const unsigned long long*>(Sq) + threadIdx.x;
    {
        unsigned long long b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) // X11: e, e + 512; L21: 1024 + e, 1024 + e + 512   (first look: cacheable, see PolledTile)
            b[q] = __hip_atomic_load(Sp + 512 * q, __ATOMIC_RELAXED, POLL_FIRST_SCOPE);
        int spins = 0;
        while (b[0] == SENT || b[1] == SENT || b[2] == SENT || b[3] == SENT) {
            if (++spins > x.spin_limit) {
                x.info[2] = 1;
                break;
            }
            poll_one(Sq + 1023, x.spin_limit, x.info);            // X11's last row
            poll_one(Sq + 1024 + 32 * 31, x.spin_limit, x.info);  // L21's last column
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (b[q] == SENT)
                    b[q] = __hip_atomic_load(Sp + 512 * q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        P2TS(6 * S + 1);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int e = threadIdx.x + 512 * q; // X11: e = k + 32 c ; L21: e = c + 32 k
            Bx[(e >> 5) * XS + (e & 31)] = __longlong_as_double((long long)b[q]);
            Ld[(e & 31) * XS + (e >> 5)] = __longlong_as_double((long long)b[2 + q]); // Ld[c][k] = L21[c][k]
        }
    }
    __syncthreads();
    double y1[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    mmk<true, 32, 2>(T, 0, Bx, 0, wm, hn, lane, y1); // Y1 = T1 X11^T
    __syncthreads();                                 // all reads of T[:, 0:32] done
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
            T[(hn + 4 * n + dcol) * PS + wm + 16 * m + drow] = y1[m][n];
    __syncthreads();
    double u[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    mmk<true, 32, 2>(T, 0, Ld, 0, wm, hn, lane, u); // Y1 L21^T
    double t2[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
            t2[m][n] = T[(32 + hn + 4 * n + dcol) * PS + wm + 16 * m + drow] - u[m][n];
    __syncthreads(); // every wave has read its part of T[:, 32:64]
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
            T[(32 + hn + 4 * n + dcol) * PS + wm + 16 * m + drow] = t2[m][n];
    if constexpr (PUBHALF) { // columns 0..31 of the strip's L tile are final: its head-tile copy starts its way now (the rest follows behind phase B)
        const int i = threadIdx.x & 63, kk0 = threadIdx.x >> 6;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int col = kk0 + 8 * q;
            __hip_atomic_store(pub + i + NB * col, T[col * PS + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (acc_on)
        mmk<false, 32, 4>(T, 0, T, 0, wm, wn, lane, a2); // the product's first half: Y1 Y1^T (columns 0..31 of T are final)
    P2TS(6 * S + 2);
    // ---- phase B: X22 ----
    {
        unsigned long long b0 = __hip_atomic_load(Sp + 2048, __ATOMIC_RELAXED, POLL_FIRST_SCOPE);
        unsigned long long b1 = __hip_atomic_load(Sp + 2048 + 512, __ATOMIC_RELAXED, POLL_FIRST_SCOPE);
        int spins = 0;
        while (b0 == SENT || b1 == SENT) {
            if (++spins > x.spin_limit) {
                x.info[2] = 1;
                break;
            }
            // (Round 4 let the one workgroup the chain waits for watch its own words instead of poll_one's: no difference,
            // 798.9 against 797.9 evaluations/s — the second look is not what a hop costs.)
            poll_one(Sq + 2048 + 1023, x.spin_limit, x.info); // X22's last row
            if (b0 == SENT)
                b0 = __hip_atomic_load(Sp + 2048, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (b1 == SENT)
                b1 = __hip_atomic_load(Sp + 2048 + 512, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const int e0 = threadIdx.x, e1 = threadIdx.x + 512; // e = k + 32 c
        Bx[(32 + (e0 >> 5)) * XS + 32 + (e0 & 31)] = __longlong_as_double((long long)b0);
        Bx[(32 + (e1 >> 5)) * XS + 32 + (e1 & 31)] = __longlong_as_double((long long)b1);
    }
    __syncthreads(); // X22 is in LDS (and T[:, 32:64] complete)
    P2TS(6 * S + 3);
    double y2[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    mmk<true, 32, 2>(T, 32, Bx + 32 * XS + 32, 0, wm, hn, lane, y2); // Y2 = T2 X22^T
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
            T[(32 + hn + 4 * n + dcol) * PS + wm + 16 * m + drow] = y2[m][n];
    __syncthreads();
    if constexpr (PUBHALF) { // ... and the other 32 columns: the product below covers most of their way
        const int i = threadIdx.x & 63, kk0 = threadIdx.x >> 6;
#pragma unroll
        for (int q = 4; q < 8; ++q) {
            const int col = kk0 + 8 * q;
            __hip_atomic_store(pub + i + NB * col, T[col * PS + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (acc_on)
        mmk<false, 32, 4>(T, 32, T, 32, wm, wn, lane, a2); // the product's second half
}

// the update of a strip's tile of column block T + 1 with the step's tile of strip T (its own: in TT; another strip's: polled)
template <int S, int ROLE, int T>
static __device__ __forceinline__ void p256_update(const P256& x, const double* __restrict__ TT, PolledTile (&hd)[3],
                                                   double (&cv)[4][8], int& nb)
{
    constexpr int CMAX = ROLE < 3 ? ROLE + 1 : 3;
    if constexpr (T >= S && T <= 2 && T + 1 <= CMAX) {
        const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const int wm = (wave & 1) * 32, wn = (wave >> 1) * 16;
        const double* Bop = TT;
        if constexpr (T != ROLE) {
            double* buf = (nb & 1) ? x.T2 : x.T1;
            ++nb;
            hd[T].finish(x.HP + (int64_t)P256_H(S, T) * (NB * NB), x.spin_limit, x.info);
            hd[T].store(buf);
            __syncthreads();
            Bop = buf;
        }
        double a2[2][4];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n)
                a2[m][n] = 0.0;
        mm64<false>(TT, Bop, wm, wn, lane, a2);
        double a2r[8];
        wave_tile_to_rows(a2, a2r, lane);
#pragma unroll
        for (int it = 0; it < 8; ++it)
            cv[T + 1][it] -= a2r[it];
    }
}

// One step of one strip.  ROLE = 0..2: the strip with that index (it factors the diagonal block of column block ROLE + 1 at the
// end of step ROLE and is done); ROLE = 3: any strip below the panel's own 256 rows.  Everything about the role is a compile-
// time constant, so that each role's code holds exactly the tiles it needs (the factorisation alone wants 192 VGPRs).
template <int S, int ROLE>
static __device__ __forceinline__ void p256_step(const P256& x, double (&cv)[4][8], double (&pr)[2][4])
{
    constexpr int CMAX = ROLE < 3 ? ROLE + 1 : 3; // last column block of the panel the strip has a tile in
    constexpr bool HEAD = ROLE <= 2;              // other strips need this strip's tile of every step
    constexpr bool CHAIN = ROLE == S && ROLE < 3; // the strip that factors next: everything it does is on the panel's critical path
    if constexpr (ROLE >= S) {
        const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const int wm = (wave & 1) * 32, wn = (wave >> 1) * 16;
        const int crow = wm + (lane & 31), ccol = wn + (lane >> 5);
        // the strip's L tile of this step: the factoring strip keeps it in T1, which its factorisation (re-carving [Bx | T0])
        // leaves alone — the tile's copy into the matrix waits until the factorisation is over
        double* const TT = CHAIN ? x.T1 : x.T0;
        if constexpr (CHAIN && S > 0) {
            double a2c[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
            p256_half_solve<S, true>(x, TT, x.T0, cv[S], a2c, true, x.S22 + (S - 1) * 3072, x.HP + (int64_t)P256_H(S, S) * (NB * NB));
            double a2r[8];
            wave_tile_to_rows(a2c, a2r, lane);
#pragma unroll
            for (int it = 0; it < 8; ++it)
                cv[S + 1][it] -= a2r[it];
            P2TS(6 * S + 5);
        }
        else {
            if constexpr (S > 0)
                p256_half_solve<S, false>(x, TT, x.T2, cv[S], pr, !HEAD && x.want_d, x.S22 + (S - 1) * 3072, nullptr);
            else {
                // ---- X_0 (from the launch before) and this strip's tile of column block 0 into LDS ----
                P2TS(6 * S + 0);
                double xv[8];
                const double* Xs = x.Xt;
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    xv[q] = Xs[threadIdx.x + 512 * q];
#pragma unroll
                for (int it = 0; it < 8; ++it)
                    TT[(ccol + 2 * it) * PS + crow] = cv[S][it];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int e = threadIdx.x + 512 * q;
                    x.Bx[(e >> 6) * XS + (e & 63)] = xv[q]; // Bx[c][k] = X[c][k]
                }
                __syncthreads();
                P2TS(6 * S + 2);
                trsm_tile_full(TT, x.Bx, lane, wave); // L_b0, ends with a barrier
                P2TS(6 * S + 3);
            }
            {
                const int i = threadIdx.x & 63, kk0 = threadIdx.x >> 6;
                double* Ag = x.A + x.R0 + (x.p0 + (int64_t)NB * S) * x.lda;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int col = kk0 + 8 * q;
                    const double v = TT[col * PS + i];
                    if constexpr (HEAD && !(CHAIN && S > 0)) // (the factoring strip's went out in two halves inside its solve)
                        __hip_atomic_store(x.HP + (int64_t)P256_H(S, ROLE) * (NB * NB) + i + NB * col, v, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT); // polled by the other strips: no flag, no acknowledgement
                    if (i < x.nrows)
                        Ag[i + (int64_t)col * x.lda] = v;
                }
            }
            if constexpr (HEAD) {
            }
            else if (S == 0 && !HEAD && x.want_d) // this strip's piece of the next panel's first diagonal block (later steps: inside the solve)
                mm64<false>(TT, TT, wm, wn, lane, pr);
            P2TS(6 * S + 4);
            if constexpr (S < 3) {
                // ---- updates of the strip's remaining column blocks c = S+1 .. CMAX with the tile of strip t = c - 1 ----
                // All tiles are asked for at once; each is completed (polled) where it is used.  Order: the strip's own tile first
                // (nothing to wait for), then highest t first — the tile of strip t = S, the one that factors next, is the last
                // to be complete.  The tiles alternate between two LDS buffers: one barrier per update.
                PolledTile hd[3];
#pragma unroll
                for (int t = 2; t >= S; --t)
                    if (t != ROLE && t + 1 <= CMAX)
                        hd[t].issue(x.HP + (int64_t)P256_H(S, t) * (NB * NB));
                int nb = 0;
                if constexpr (HEAD && !CHAIN)
                    p256_update<S, ROLE, ROLE>(x, TT, hd, cv, nb); // with its own tile first: the polled ones are on their way meanwhile
                if constexpr (ROLE != 2)
                    p256_update<S, ROLE, 2>(x, TT, hd, cv, nb);
                if constexpr (S <= 1 && ROLE != 1)
                    p256_update<S, ROLE, 1>(x, TT, hd, cv, nb);
                if constexpr (S == 0 && ROLE != 0)
                    p256_update<S, ROLE, 0>(x, TT, hd, cv, nb);
                if constexpr (CHAIN)
                    p256_update<S, ROLE, ROLE>(x, TT, hd, cv, nb); // (S = 0 only: later steps update inside the solve)
                if constexpr (!CHAIN)
                    __syncthreads(); // T0 and the buffers are free again
            }
            P2TS(6 * S + 5);
        }
        if constexpr (CHAIN) {
            // ---- tile S + 1 is the finished diagonal block of column block S + 1 ----
            __syncthreads();   // [Bx | T0] have no readers left
            double* Ls = x.Bx; // [Ls | Ltb | invd | sync | Xw] re-carved over [Bx | T0], as in k_panel_step; T1 = this strip's L tile
            double* Ltb = Ls + NB * XS;
            double* invd = Ltb + DIAG_LTB;
#pragma unroll
            for (int it = 0; it < 8; ++it)
                Ls[crow * XS + ccol + 2 * it] = cv[S + 1][it];
            DiagSync* sy = reinterpret_cast<DiagSync*>(invd + NB);
            diag_flow_init(sy);
            __syncthreads();
            P2TS(26);
            DiagEarly ea;
            ea.mute = x.mute;
            ea.S = x.S22 + S * 3072;
            diag_flow(Ls, Ltb, invd, sy, x.A + x.R0 + x.R0 * x.lda, x.lda, x.Xt + (S + 1) * (NB * NB), x.info, x.R0, wave, lane,
                      invd + NB + 8, &ea);
            P2TS(27);
            __syncthreads(); // (the tile in T1 is still to be copied into the matrix: after every wave's part of the factorisation)
            P2TS(28);
            P2TS(29);
            if constexpr (S > 0) { // this strip's L tile of the step into the matrix: nobody reads it there before the launch ends
                const int i = threadIdx.x & 63, kk0 = threadIdx.x >> 6;
                double* Ag = x.A + x.R0 + (x.p0 + (int64_t)NB * S) * x.lda;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int col = kk0 + 8 * q;
                    Ag[i + (int64_t)col * x.lda] = TT[col * PS + i];
                }
            }
        }
    }
}

template <int ROLE>
static __device__ __forceinline__ void p256_strip(const P256& x, double* __restrict__ Dacc)
{
    constexpr int CMAX = ROLE < 3 ? ROLE + 1 : 3;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 16;
    // the strip's tiles, lane = row layout (wave_tile_to_rows): element it of a thread is row wm + (lane & 31), column
    // wn + 2 it + (lane >> 5) of the 64 x 64 tile
    const int crow = wm + (lane & 31), ccol = wn + (lane >> 5);
    const int crc = crow < x.nrows ? crow : x.nrows - 1;
    double cv[4][8];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int it = 0; it < 8; ++it)
            cv[c][it] = (c <= CMAX) ? x.A[x.R0 + crc + (x.p0 + (int64_t)NB * c + ccol + 2 * it) * x.lda] : 0.0;
    double pr[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
            pr[m][n] = 0.0;
    p256_step<0, ROLE>(x, cv, pr);
    p256_step<1, ROLE>(x, cv, pr);
    p256_step<2, ROLE>(x, cv, pr);
    p256_step<3, ROLE>(x, cv, pr);
    if constexpr (ROLE == 3) {
        if (x.want_d) {
            double prr[8];
            wave_tile_to_rows(pr, prr, lane);
#pragma unroll
            for (int it = 0; it < 8; ++it)
                Dacc[threadIdx.x + 512 * it] = prr[it];
        }
    }
}

__global__ __launch_bounds__(512) void k_panel256(double* __restrict__ A, int64_t lda, int64_t p0, int64_t M,
                                                  double* __restrict__ Xt, int* __restrict__ info, int64_t dnext,
                                                  double* __restrict__ Dacc, int spin_limit, double* __restrict__ S22,
                                                  double* __restrict__ S22_next)
{
    __shared__ __attribute__((aligned(16))) double lds[NB * XS + 3 * NB * PS]; // [Bx | T0 | T1 | T2]: 156,672 B
    static_assert(NB * XS + DIAG_LTB + NB + 8 + DIAG_XW_DOUBLES <= NB * XS + NB * PS, "the factoring strips' carve fits into [Bx | T0]");
    const int b = (int)blockIdx.x;
    P256 x;
    x.A = A;
    x.lda = lda;
    x.p0 = p0;
    x.R0 = p0 + (int64_t)NB * (b + 1);
    x.Xt = Xt;
    x.info = info;
    x.mute = spin_limit < 0; // test hook (GPE_HANDOVER_FAULT): nobody publishes, every consumer gives up at once
    x.spin_limit = spin_limit < 0 ? -spin_limit : spin_limit;
    x.nrows = (int)((M - x.R0 < NB) ? M - x.R0 : NB);
    x.want_d = dnext >= 0 && x.R0 == dnext;
    x.Bx = lds;
    x.T0 = lds + NB * XS;
    x.T1 = x.T0 + NB * PS;
    x.T2 = x.T1 + NB * PS;
    x.S22 = S22;
    x.HP = S22 + P256_POLLED_S;
    { // the polled copies of the NEXT launch start from the all-ones pattern (this launch's were armed by the one before: same
      // stream, complete before this one began); a quarter each for the last four strips
        unsigned long long* nx = reinterpret_cast<unsigned long long*>(S22_next);
        constexpr int QUARTER = P256_POLLED_DOUBLES / 4;
#pragma unroll
        for (int part = 0; part < 4; ++part) {
            const int owner = (int)gridDim.x - 1 - part > 0 ? (int)gridDim.x - 1 - part : 0;
            if (b == owner)
                for (int idx = threadIdx.x; idx < QUARTER; idx += 512)
                    nx[part * QUARTER + idx] = ~0ull;
        }
    }
    P2TS(30);
    switch (b) {
    case 0: p256_strip<0>(x, Dacc); break;
    case 1: p256_strip<1>(x, Dacc); break;
    case 2: p256_strip<2>(x, Dacc); break;
    default: p256_strip<3>(x, Dacc); break;
    }
    P2TS(31);
}

static std::atomic<gpe_epoch_t> g_handover_epoch{0}; // a value no earlier launch of this process has used; 64 bits: never wraps

void launch_panel256(hipStream_t s, double* A, int64_t lda, int64_t p0, int64_t M, double* Xt, int* info, int64_t dnext,
                     double* Dacc, double* S22, double* S22_next, hipEvent_t stop)
{
    const int spin_limit = flow_spin_limit();
    const int64_t rows = M - (p0 + NB);
    if (rows <= 0)
        return;
    const dim3 grid((unsigned)((rows + NB - 1) / NB)), block(512);
    FlowGate gate(s); // (its strips poll each other inside the launch: dev.h)
    if (stop)
        GPE_LAUNCH_STOP("k_panel256", k_panel256, grid, block, 0, s, stop, A, lda, p0, M, Xt, info, dnext, Dacc, spin_limit, S22, S22_next);
    else
        GPE_LAUNCH(k_panel256, grid, block, 0, s, A, lda, p0, M, Xt, info, dnext, Dacc, spin_limit, S22, S22_next);
}

// ---------------------------------------------------------------------------------------------
// k_upd_fused — the next-panel update (rows >= pe of columns [pe, pe2), k = pe - p0) and, in the SAME
// launch, the factorisation of the next diagonal block.  The update is the 64 x 64 direct-to-LDS GEMM
// (gemm_glds64.h) on gridDim.x - 1 workgroups, which leave tile (0, 0) alone; the last workgroup forms
// that tile itself — A[pe:pe+64, pe:pe+64] - L_d L_d^T with L_d = A[pe:pe+64, p0:pe], (pe - p0) / 64
// products of 64^3 — and then factors and half-inverts it exactly like workgroup 0 of k_panel_step.
// k_diag used to follow the update as a launch of its own (13.6 us on the critical path of every
// outer panel, with 255 CUs idle); here it runs underneath the update (~18 us).
// (Round 3 also folded the panel's last 64-column step into this launch — UpdFold — for the step-by-step panels; the
// one-launch panels made it unreachable and round 4 removed it.)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void k_upd_fused(GemmArgs g, double* __restrict__ A, int64_t lda, int64_t p0, int64_t pe,
                                                   double* __restrict__ Xt_next, int* __restrict__ info,
                                                   const double* __restrict__ Dacc)
{
    constexpr int GEMM_LDS = 4 * Glds64Shape<16>::STAGE, DIAG_LDS = 2 * NB * PS;
    constexpr int LDS_DOUBLES = GEMM_LDS > DIAG_LDS ? GEMM_LDS : DIAG_LDS;
    __shared__ __attribute__((aligned(16))) double lds[LDS_DOUBLES]; // the update's 4 operand stages / the diagonal workgroup's tiles
    if (blockIdx.x + 1 < gridDim.x) {
        gemm_glds64_body<16, 4, 8>(g, lds, (int)blockIdx.x, (int)gridDim.x - 1, true);
        return;
    }
    // ---- the diagonal workgroup ----
    static_assert(NB * XS + DIAG_LTB + NB + 8 + DIAG_XW_DOUBLES <= 2 * NB * PS,
                  "[Ls | Ltb | invd | sync | Xw] is carved out of the two operand tiles");
    double* T0 = lds;
    double* T1 = lds + NB * PS;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 16;
    const int crow = wm + (lane & 31), ccol = wn + (lane >> 5);
    double c0v[8]; // the tile before the update, lane = row layout
#pragma unroll
    for (int it = 0; it < 8; ++it)
        c0v[it] = A[pe + crow + (pe + ccol + 2 * it) * lda];
    const int nkb = (int)((pe - p0) / NB); // 0: the panel steps already applied every piece (k_panel_step, dnext)
    TileRegs tl;
    if (nkb > 0)
        tl.load(A + pe + p0 * lda, lda, NB);
    double acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
            acc[m][n] = 0.0;
#pragma unroll 1
    for (int c = 0; c < nkb; ++c) { // two tiles alternate: a wave that refills one has passed the barrier behind its last readers
        double* T = (c & 1) ? T1 : T0;
        tl.store(T);
        if (c + 1 < nkb)
            tl.load(A + pe + (p0 + (int64_t)NB * (c + 1)) * lda, lda, NB);
        __syncthreads();
        mm64<false>(T, T, wm, wn, lane, acc);
    }
    __syncthreads(); // the operand tiles are dead: re-carve
    double* Ls = lds;
    double* Ltb = Ls + NB * XS;
    double* invd = Ltb + DIAG_LTB;
    {
        double a2r[8];
        wave_tile_to_rows(acc, a2r, lane);
#pragma unroll
        for (int it = 0; it < 8; ++it) // Dacc: what the panel steps summed up (same thread <-> element mapping)
            Ls[crow * XS + ccol + 2 * it] = c0v[it] - a2r[it] - (Dacc ? Dacc[threadIdx.x + 512 * it] : 0.0);
    }
    {
        DiagSync* sy = reinterpret_cast<DiagSync*>(invd + NB);
        diag_flow_init(sy);
        __syncthreads();
        diag_flow(Ls, Ltb, invd, sy, A + pe + pe * lda, lda, Xt_next, info, pe, wave, lane, invd + NB + 8);
        return;
    }
}

// g: the next-panel update as for launch_gemm_sub (tri, 64-multiple shapes checked by the caller)
void launch_upd_fused(hipStream_t s, const GemmArgs& g0, double* A, int64_t lda, int64_t p0, int64_t pe, double* Xt_next,
                      int* info, const double* Dacc)
{
    constexpr int TM = 64, TN = 64;
    GemmArgs g = g0;
    const int tiles_m = (int)((g.m + TM - 1) / TM), tiles_n = (int)((g.n + TN - 1) / TN);
    int fold = 1;
    const int nsup = (tiles_n + 1) / 2;
    for (int sc = 0; sc < nsup; ++sc) { // live-tile enumeration of gemm.hip:launch_glds64
        const int t2 = tiles_n - 1 - sc;
        int len = tiles_m - first_live_tile<TM, TN>(g, sc);
        if (t2 != sc)
            len += tiles_m - first_live_tile<TM, TN>(g, t2);
        fold = len > fold ? len : fold;
    }
    g.fold_len = fold;
    g.total = nsup * fold;
    const dim3 grid((unsigned)g.total + 1), block(512);
    if (g.stop_event)
        GPE_LAUNCH_STOP("k_upd_fused", k_upd_fused, grid, block, 0, s, (hipEvent_t)g.stop_event, g, A, lda, p0, pe, Xt_next, info, Dacc);
    else
        GPE_LAUNCH(k_upd_fused, grid, block, 0, s, g, A, lda, p0, pe, Xt_next, info, Dacc);
}

#ifdef DIAG_TIMING
void dump_diag_timing()
{
    long long h[32];
    hipMemcpyFromSymbol(h, HIP_SYMBOL(g_diag_ts), sizeof(h));
    printf("k_diag cycles: load %lld | factor + invert %lld | total %lld\n", h[1] - h[0], h[2] - h[1], h[2] - h[0]);
}
void dump_p256_timing()
{
    long long h[5][32];
    hipMemcpyFromSymbol(h, HIP_SYMBOL(g_p256_ts), sizeof(h));
    const char* names[5] = {"strip 0", "strip 1", "strip 2", "strip 3", "last strip"};
    long long t0 = h[0][30];
    for (int r = 0; r < 5; ++r)
        t0 = h[r][30] < t0 ? h[r][30] : t0;
    // wall_clock64 (s_memrealtime): the 100 MHz constant clock, the same on every CU -> 10 ns units
    printf("k_panel256 stamps (us after the first strip's start; per step: enter | X flag seen | X+tile in LDS | solved | L out/published | updates done)\n");
    for (int r = 0; r < 5; ++r) {
        printf("  %-10s start %6.2f :", names[r], (h[r][30] - t0) * 0.01);
        const int smax = r < 3 ? r : 3;
        for (int S = 0; S <= smax; ++S) {
            printf(" [S%d", S);
            for (int i = 0; i < 6; ++i)
                if (!(S == 0 && i == 1))
                    printf(" %6.2f", (h[r][6 * S + i] - t0) * 0.01);
            printf("]");
        }
        if (r < 3)
            printf(" diag start %6.2f wave 0 done %6.2f all acked %6.2f X out %6.2f", (h[r][26] - t0) * 0.01, (h[r][27] - t0) * 0.01,
                   (h[r][28] - t0) * 0.01, (h[r][29] - t0) * 0.01);
        printf(" end %6.2f\n", (h[r][31] - t0) * 0.01);
    }
}
void dump_panel_timing()
{
    long long h[64];
    hipMemcpyFromSymbol(h, HIP_SYMBOL(g_panel_ts), sizeof(h));
    printf("k_panel_step WG0 cycles: loads %lld | trsm %lld | writeL %lld | updates %lld | to-diag %lld | rounds %lld | tail %lld | total %lld\n",
           h[1] - h[0], h[2] - h[1], h[3] - h[2], h[4] - h[3], h[5] - h[4], h[6] - h[5], h[7] - h[6], h[7] - h[0]);
    printf("k_panel_step last WG cycles: loads %lld | trsm %lld | writeL %lld | updates %lld | total %lld\n", h[33] - h[32],
           h[34] - h[33], h[35] - h[34], h[36] - h[35], h[36] - h[32]);
    printf("  its first update (wave 0): wait + fetch head tiles %lld | tile -> LDS + barrier %lld | 64^3 product %lld | to row layout %lld | C -= , store %lld | barrier %lld\n",
           h[42] - h[35], h[43] - h[42], h[44] - h[43], h[45] - h[44], h[46] - h[45], h[47] - h[46]);
}
#endif
void launch_panel_step(hipStream_t s, double* A, int64_t lda, int64_t j0, int64_t M, int nt, const double* Xt_cur,
                       double* Xt_next, int do_next, int* info, double* Hs, int64_t dnext, int64_t dfirst, int dinit,
                       double* Dacc, gpe_epoch_t* hflag)
{
    // a value no earlier launch of this process has used (0 is what fresh flag words hold)
    const gpe_epoch_t epoch = ++g_handover_epoch;
    const int spin_limit = flow_spin_limit();
    const int64_t rows = M - (j0 + NB);
    if (rows <= 0)
        return;
    // (No FlowGate here: the consumers of this launch wait for its FIRST workgroups only, a batch of 64 members runs two
    // sub-batches of these steps on two streams on purpose — one's panel steps under the other's updates, 8.9 k against 7.9 k
    // evaluations/s with the steps ordered — and two rounds of that have not seen a lost hand-over; the polls are bounded.)
    if (g_batch.bt)
        GPE_LAUNCH(k_panel_step_b, dim3((unsigned)((rows + NB - 1) / NB) * g_batch.G), dim3(512), 0, s, A, lda, j0, M, nt,
                           Xt_cur, Xt_next, do_next, info, Hs, dnext, dfirst, dinit, Dacc, hflag, epoch, spin_limit, g_batch.bt);
    else
        GPE_LAUNCH(k_panel_step, dim3((unsigned)((rows + NB - 1) / NB)), dim3(512), 0, s, A, lda, j0, M, nt, Xt_cur,
                           Xt_next, do_next, info, Hs, dnext, dfirst, dinit, Dacc, hflag, epoch, spin_limit);
}

// head tiles of the fused steps of one outer panel -> their place in A.  Step f (f = 0..nf-1) of the
// panel starting at column p0 left nt0 - f tiles: tile t = rows p0 + 64 (f + 1 + t), columns p0 + 64 f.
__global__ __launch_bounds__(256) void k_head_copy(double* __restrict__ A, int64_t lda, int64_t p0, int nt0,
                                                   const double* __restrict__ H, const BatchTab* __restrict__ bt)
{
    BT_REBASE(bt, A);
    BT_REBASE(bt, H);
    int f = 0, t = blockIdx.x;
    while (t >= nt0 - f) {
        t -= nt0 - f;
        ++f;
    }
    const double* src = H + (int64_t)blockIdx.x * (NB * NB);
    double* dst = A + (p0 + NB * (int64_t)(f + 1 + t)) + (p0 + NB * (int64_t)f) * lda;
    for (int e = threadIdx.x; e < NB * NB; e += 256)
        dst[(e & 63) + (int64_t)(e >> 6) * lda] = src[e];
}
void launch_head_copy(hipStream_t s, double* A, int64_t lda, int64_t p0, int nt0, int nf, const double* H)
{
    int tiles = 0;
    for (int f = 0; f < nf; ++f)
        tiles += nt0 - f;
    if (tiles > 0)
        GPE_LAUNCH(k_head_copy, dim3((unsigned)tiles, 1, g_batch.G), dim3(256), 0, s, A, lda, p0, nt0, H, g_batch.bt);
}
