// dev.h — internal declarations shared by the HIP translation units of libgpengine.so.
// gfx950 (MI355X, CDNA4) only: wave = 64 lanes, v_mfma_f64_16x16x4_f64, 160 KiB LDS/CU.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdlib.h>
#include "shell_layout.h" // (the regions of a handle's two shell blocks; GPE_MAX_P and k_panel256's polled buffer size with them)

// ---- environment switches (SWITCHES.md); callers keep the result in a function-local static: read once per process ----
// an integer switch: its value, or dflt when it is not set
static inline int64_t env_int(const char* name, int64_t dflt)
{
    const char* e = getenv(name);
    return e ? atoll(e) : dflt;
}
// an on/off switch: on unless it is set to 0 / dflt when it is not set
static inline bool env_flag(const char* name, bool dflt) { return env_int(name, dflt) != 0; }
static inline bool env_not_zero(const char* name) { return env_flag(name, true); }

#define GPE_MAX_THETA 64
#define GPE_MAX_DEVICES 16 // per-device tables of the host side (shell pool, gate, live handles, batch tables) have this many entries

// kernel-functor parameters, pre-digested on the host (kernel/kernel.hpp:116-123 and the
// per-kernel set_params: squared_exp_ard.hpp:96-105, matern_five_halves.hpp:97-102)
struct KParams {
    int kind;  // gpe_kernel_kind
    int D;     // rows of the SoA sample matrix that enter the distance: input dimension (+ k projection rows, below)
    int Din;   // input dimension
    int k_lam; // SE-ARD with M = Lambda Lambda^T + diag(ell^-2), Lambda D x k (squared_exp_ard.hpp:109-126,142-146):
               // rows Din .. Din+k-1 of the sample matrix hold the projections Lambda^T x (inv_ell = 1 there), so
               // (x1-x2)^T M (x1-x2) is the same sum of squares over D = Din + k rows
    double sf2;                 // sigma_f^2 = exp(2 p_last)
    double inv_l;               // 1/l (isotropic kernels)
    double diag_add;            // noise + 1e-8 (kernel.hpp:83)
    double noise;               // sigma_n^2
    double inv_ell[GPE_MAX_THETA]; // 1/ell_d (SE-ARD)
};

typedef double d4_t __attribute__((ext_vector_type(4)));

static __device__ __forceinline__ d4_t mfma_f64(double a, double b, d4_t c)
{
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// ---- batched launches: G independent GPs of the same shape stepped by ONE launch per stage ------------------------
// (multi_gp.hpp:124-126 / parallel_repeater.hpp:86-105 as gpe_batch_compute runs them: config 4, 64 x N = 2048.)
// Every GP has its own buffers, allocated separately.  The launch sequence is built once, from GP 0's pointers, with
// gridDim.z = G; workgroup z translates each pointer argument from GP 0's buffer into GP z's buffer of the same class
// (wave-uniform: a handful of scalar compares per pointer).  The per-GP kernel parameters travel in the same table.
#define GPE_BT_CLS 13
#define GPE_BT_MAXG 64
struct BatchTab {
    int G;
    int ncls;
    const char* base0[GPE_BT_CLS];              // GP 0's buffers ...
    unsigned long long size[GPE_BT_CLS];         // ... and their sizes in bytes
    const char* base[GPE_BT_CLS][GPE_BT_MAXG];   // the same buffer of every GP
    KParams kp[GPE_BT_MAXG];
};
template <class T>
static __device__ __forceinline__ T* bt_rebase(const BatchTab* __restrict__ bt, int g, T* p)
{
    const char* q = (const char*)p;
#pragma unroll
    for (int c = 0; c < GPE_BT_CLS; ++c) {
        const unsigned long long off = (unsigned long long)(q - bt->base0[c]);
        if (off < bt->size[c])
            return (T*)(bt->base[c][g] + off);
    }
    return p;
}
#define BT_REBASE(bt, p)                          \
    do {                                          \
        if (bt)                                   \
            p = bt_rebase(bt, (int)blockIdx.z, p); \
    } while (0)
// what the launch wrappers of this thread add to every launch (set by gpe_batch_compute around the enqueue)
struct BatchLaunch {
    const BatchTab* bt = nullptr; // device copy
    int G = 1;
};
extern thread_local BatchLaunch g_batch;

// the kernel functors' value from z = sum_d ((x1_d - x2_d) / ell_d)^2 (kbuild.hip, small.hip)
static __device__ __forceinline__ double kfun(int kind, double z, double sf2)
{
    // z = sum_d ((x1_d - x2_d) / ell_d)^2   (isotropic kernels: ell_d = l for every d)
    switch (kind) {
    case 0: // SquaredExpARD::kernel, squared_exp_ard.hpp:148-150
    case 3: // Exp::kernel, exp.hpp:97-102
        return sf2 * exp(-0.5 * z);
    case 1: { // MaternFiveHalves::kernel, matern_five_halves.hpp:104-113
        double r = sqrt(z);
        double term1 = 2.23606797749978969641 * r; // sqrt(5) d / l
        double term2 = (5.0 / 3.0) * z;            // 5 d^2 / (3 l^2)
        return sf2 * (1.0 + term1 + term2) * exp(-term1);
    }
    default: { // MaternThreeHalves::kernel, matern_three_halves.hpp:101-107
        double term = 1.73205080756887729353 * sqrt(z);
        return sf2 * (1.0 + term) * exp(-term);
    }
    }
}

// ---- workgroup -> unknown block of a one-launch data-flow sweep (solve.hip, solve_mp.hip) ------------------
// Two requirements meet here.  (1) Progress without assuming that every workgroup is resident: a workgroup may
// only ever wait for workgroups with a LOWER blockIdx.x — the dispatcher hands workgroups out in that order, so
// whatever a resident workgroup polls for is resident or finished, however many CUs other streams (other handles'
// sweeps, 147 KB-LDS GEMMs) hold.  (2) Consecutive blocks of the chain on one XCD (hops served by that XCD's L2).
// The dispatcher deals blockIdx.x round-robin over the 8 XCDs, so a grid of nblk workgroups cannot have both.
// The grid therefore has 8 workgroups per chain position s = blockIdx.x / 8 (s-th block to be solved: s going up
// for the forward sweep, nblk-1-s for the backward one); only the one that sits on the XCD owning that block's
// contiguous range of the chain works, the other seven return at once (-1).
#define GPE_FLOW_SPIN_LIMIT (1 << 22) // bounded poll: ~a second; raises *err, and the host re-runs block by block
// (bx of gx: the workgroup's place in ITS chain's grid — blockIdx.x of gridDim.x for a single GP; a batched sweep interleaves its
// members' chains in one 1-D grid, batch.hpp / solve.hip)
static __device__ __forceinline__ int64_t flow_block_of_at(int64_t nblk, bool backward, int64_t bx, int64_t gx)
{
    if (gx == nblk) // plain form (GPE_FLOW_XCD=0, batched sweeps): chain position = dispatch position, no XCD locality
        return backward ? nblk - 1 - bx : bx;
    const int64_t s = bx >> 3;
    const int64_t x = bx & 7;
    const int64_t j = backward ? nblk - 1 - s : s;
    const int64_t q = nblk / 8, r = nblk % 8, split = r * (q + 1);
    const int64_t owner = j < split ? j / (q + 1) : r + (j - split) / (q > 0 ? q : 1);
    return x == owner ? j : -1;
}
static __device__ __forceinline__ int64_t flow_block_of(int64_t nblk, bool backward)
{
    return flow_block_of_at(nblk, backward, (int64_t)blockIdx.x, (int64_t)gridDim.x);
}
unsigned flow_grid(int64_t nblk); // 8 nblk (XCD-local chains) or nblk (GPE_FLOW_XCD=0)
#define GPE_FLOW_GRID(nblk) flow_grid(nblk)

// ---- launch tracing (GPE_TRACE=1 / gpe_trace(1)) ------------------------------------------------------------------
// rocprofv3's kernel trace delays every dispatch that carries its own completion event by ~100 us, so the PRODUCTION
// schedule of the factorisation (look-ahead on two streams, the fused next-panel update + diagonal block) cannot be traced
// with it.  With tracing on, every launch of the library carries a start and a stop event of its own instead
// (hipExtLaunchKernelGGL: the dispatch packet's own timestamps, no marker packets, the mechanism the look-ahead already
// uses for ordering), and gpe_trace_dump() writes (kernel, stream, start, end) relative to the first launch.
bool gpe_trace_on();
hipEvent_t gpe_trace_event();
void gpe_trace_add(const char* name, hipStream_t s, hipEvent_t e0, hipEvent_t e1, dim3 grid, dim3 block);
#define GPE_LAUNCH_NAMED(name, kern, grid, block, shmem, stream, ...)                                      \
    do {                                                                                                   \
        if (gpe_trace_on()) {                                                                              \
            hipEvent_t e0_ = gpe_trace_event(), e1_ = gpe_trace_event();                                   \
            hipExtLaunchKernelGGL(kern, grid, block, shmem, stream, e0_, e1_, 0, __VA_ARGS__);             \
            gpe_trace_add(name, stream, e0_, e1_, grid, block);                                            \
        }                                                                                                  \
        else                                                                                               \
            hipLaunchKernelGGL(kern, grid, block, shmem, stream, __VA_ARGS__);                             \
    } while (0)
#define GPE_LAUNCH(kern, grid, block, shmem, stream, ...) GPE_LAUNCH_NAMED(#kern, kern, grid, block, shmem, stream, __VA_ARGS__)
// the same for a launch that signals `stop` (an event of the caller's: the look-ahead's ordering) through its dispatch
#define GPE_LAUNCH_STOP(name, kern, grid, block, shmem, stream, stop, ...)                                 \
    do {                                                                                                   \
        if (gpe_trace_on()) { /* (the caller's event has no timestamps: own events + a marker packet for `stop`) */ \
            hipEvent_t e0_ = gpe_trace_event(), e1_ = gpe_trace_event();                                   \
            hipExtLaunchKernelGGL(kern, grid, block, shmem, stream, e0_, e1_, 0, __VA_ARGS__);             \
            hipEventRecord(stop, stream);                                                                  \
            gpe_trace_add(name, stream, e0_, e1_, grid, block);                                            \
        }                                                                                                  \
        else                                                                                               \
            hipExtLaunchKernelGGL(kern, grid, block, shmem, stream, nullptr, stop, 0, __VA_ARGS__);        \
    } while (0)

// ---- kernel-matrix build (kbuild.hip) ----------------------------------------------
// Xt: SoA, D x ldx (sample index contiguous).  Writes the LOWER triangle (incl. diagonal,
// + diag_add) of K into A (col-major, lda).  gp.hpp:556-558 + kernel.hpp:81-84.
// tail (optional): what launch_cols_to_rows does, by extra workgroups of the same launch (kbuild.hip); returns whether it was
// taken (the wide build kernel, single-GP launches) — otherwise the caller launches it itself
struct BuildRowsTail {
    const double* V; // N x P (ld ldv)
    int64_t ldv;
    int P;
    double* Arows;   // A + N: row p of column i at Arows[p + i * lda]
    double* sent;    // optional, as for launch_cols_to_rows
    int64_t first;   // (set by the launcher)
};
bool launch_build_K(hipStream_t s, const double* Xt, int64_t ldx, int64_t N, const KParams& kp,
                    double* A, int64_t lda, const BuildRowsTail* tail = nullptr);
// full symmetric K (tests / gpe_get_K)
void launch_build_K_full(hipStream_t s, const double* Xt, int64_t ldx, int64_t N, const KParams& kp,
                         double* A, int64_t lda);
// cross kernel Ks[i, m] = k(x_i, q_m), no noise (gp.hpp:626-632); Qt SoA D x ldq; Ks col-major N x M
void launch_build_Ks(hipStream_t s, const double* Xt, int64_t ldx, int64_t N, const double* Qt, int64_t ldq,
                     int64_t M, const KParams& kp, double* Ks, int64_t ldk);
// kvv[m] = k(q_m, q_m)
void launch_kvv(hipStream_t s, const double* Qt, int64_t ldq, int64_t M, const KParams& kp, double* kvv);
// row-major (n x D) -> SoA (D x ld), writing columns [col0, col0+n)
void launch_transpose_x(hipStream_t s, const double* Xrm, int64_t n, int D, double* Xt, int64_t ld, int64_t col0);
// Lambda (D x k, column-major as in the parameter vector: squared_exp_ard.hpp:100-102)
struct LamParams {
    int D, k;
    double A[GPE_MAX_THETA];
};
// rows D .. D+k-1 of Xt, columns [col0, col0+n):  Xt[(D+j) ld + i] = sum_d A[d + j D] Xt[d ld + i]
void launch_lambda_rows(hipStream_t s, double* Xt, int64_t ld, int64_t col0, int64_t n, const LamParams& lp);

// ---- Cholesky diagonal block (potrf.hip; the panel launches: potrf_panel.hip) --------------------------------------------
// factor the jb x jb (jb <= 64) diagonal block at A (in place, lower) and write the transposed
// inverse Xt[k + 64 c] = (L11^-1)[c][k] (64 x 64, identity-padded for jb < 64).  info: first bad
// pivot (1-based, global index = goff + j + 1): the word takes the minimum of what is reported
// (diag_flow.h: report_pivot; the ragged block's round kernel, alone in its launch, writes if *info == 0).
// half_form (jb == 64 only): only the inverses of the two 32 x 32 diagonal half-blocks are produced
// (round 1; the data-flow block kernel of diag_flow.h leaves ALL of the inverse and ignores the flag).
void launch_diag(hipStream_t s, double* A, int64_t lda, int jb, double* Xt, int* info, int64_t goff, int half_form);
// one fused 64-column step below the factored diagonal block at (j0, j0): L21 = A21 X^T for rows
// j0+64 .. M-1, the updates of the next `nt` 64-column blocks of the outer panel, and (do_next) the
// factorisation + inversion of the next diagonal block (-> Xt_next).  Full 64-blocks only.
typedef shell::flag_t gpe_epoch_t; // the value of a hand-over flag word: the serial number of the launch that set it
// Hs: nt scratch tiles (64 x 64 each) for the L of the first nt row blocks; launch_head_copy moves
// the tiles of the nf fused steps of the panel at p0 (nt0 = tiles of its first step) into A.
// dnext / dfirst (>= 0 to enable): see k_panel_step — pieces of the next outer panel's first diagonal block
void launch_panel_step(hipStream_t s, double* A, int64_t lda, int64_t j0, int64_t M, int nt, const double* Xt_cur,
                       double* Xt_next, int do_next, int* info, double* Hs, int64_t dnext, int64_t dfirst, int dinit,
                       double* Dacc, gpe_epoch_t* hflag);
// all steps of the 256-column outer panel at p0 in one launch (potrf_panel.hip: k_panel256); Xt = inverse of the diagonal block at
// p0 (the next three follow at + 4096 each and are written), dnext / Dacc as above
void launch_panel256(hipStream_t s, double* A, int64_t lda, int64_t p0, int64_t M, double* Xt, int* info, int64_t dnext,
                     double* Dacc, double* S22, double* S22_next, hipEvent_t stop = nullptr);
// nt tile columns of a panel of nb row strips in one data-flow launch (potrf_tail.hip: k_tail) — the closing columns of the
// factorisation (nb = nt [+ 1 for the right-hand-side rows]) or a tall head panel (nb > nt); a buffer = the polled quarters
// of nt block inverses, then a slot per tile
#define GPE_TAIL_MAX 8192 // (upper bound of the setting; the default: engine.hip)
// Data-flow launches (k_tail, k_panel256, the one-launch sweeps) wait INSIDE the launch for lower-numbered workgroups of the same
// launch.  That is deadlock-free for one such launch at a time — its lowest unfinished workgroup is always resident — but not
// for two from different streams: each XCD dispatches its share of every launch in order, and the CUs of the XCD that the
// lowest unfinished workgroup of launch A belongs to can all be held by waiting workgroups of launch B and vice versa (round
// 4: four handles evaluated from four host threads ran into the bounded polls and the re-run path, 1 evaluation/s instead of
// 1300; profiles/r04_concurrent_flow_launches.log).  So a data-flow launch from one stream waits for the previous one on the
// device when that one went to another stream (an event recorded at that stream's end at that moment; nothing otherwise).  engine.hip.
void flow_gate_enter(hipStream_t s);
void flow_gate_leave(hipStream_t s);
void flow_gate_forget(hipStream_t s);
struct FlowGate {
    hipStream_t s;
    bool on;
    explicit FlowGate(hipStream_t s_, bool engage = true) : s(s_), on(engage)
    {
        if (on)
            flow_gate_enter(s);
    }
    ~FlowGate()
    {
        if (on)
            flow_gate_leave(s);
    }
    FlowGate(const FlowGate&) = delete;
    FlowGate& operator=(const FlowGate&) = delete;
};
int debug_tail_order(int nt, int nb, int lag, int pair); // potrf_tail.hip (host only)
void debug_chain_split(int wave, int* units10, int* cols); // potrf_tail.hip (host only): the chain workgroup's work split
static inline int64_t tail_tiles(int64_t nt, int64_t nb) { return nt * nb - nt * (nt - 1) / 2; }
static inline int64_t tail_buf_doubles(int64_t nt, int64_t nb) { return nt * 3072 + tail_tiles(nt, nb) * 4096; }
// gen (optional): the launch generates its tiles of K from the samples (and obs_mean's rows from Om) instead of reading A,
// and pre-fills the sweep's sentinel in Al for its columns — no kernel-matrix build in front of it
struct TailGen {
    const double* Xg; // SoA samples
    int64_t ldx, Ns;
    const double* Om;
    int64_t ldom;
    double* Al; // may be null
    int64_t ldal;
    int P;
    const KParams* kp; // host copy (single launches pass it by value; batched ones read the batch table)
};
int ragged_split(int64_t k, int64_t scratch_doubles, int* kc_out); // potrf_tail.hip (host only)
bool launch_ragged_finish(hipStream_t s, double* C, int64_t ldc, const double* A, int64_t ld, int64_t jb, int64_t P, int64_t k,
                          double* scratch, int64_t scratch_doubles, double* Xt, int* info, int64_t goff); // potrf_tail.hip: update + factor + solve
bool launch_ragged_update(hipStream_t s, double* C, int64_t ldc, const double* A, int64_t ld, int64_t m, int64_t n, int64_t k,
                          double* scratch, int64_t scratch_doubles); // potrf_tail.hip: a ragged order's last block behind k_tail
void launch_tail(hipStream_t s, double* A, int64_t lda, int64_t t0, int64_t t1, int64_t N64, int64_t M, double* Xt_all, int* info,
                 double* buf_cur, double* buf_next, const TailGen* gen = nullptr);
// S22 / S22_next: the polled hand-over buffers (block inverses + head tiles), P256_POLLED_DOUBLES each, holding the all-ones
// pattern when the launch starts (the launch arms S22_next); they are shell::s22 of either half of the head block, and Dacc
// and hflag of the panel launches shell::diag_sum and shell::hflags (shell_layout.h)
void launch_head_copy(hipStream_t s, double* A, int64_t lda, int64_t p0, int nt0, int nf, const double* H);
// inverses of diagonal blocks b0 .. b0+nblocks-1 of an existing factor L (order N) into
// Xt_all + 4096 b
void launch_diag_inv(hipStream_t s, const double* L, int64_t ldl, int64_t N, int64_t b0, int64_t nblocks,
                     double* Xt_all);

// ---- fp64 MFMA GEMM update (gemm.hip) ----------------------------------------------
// C[m x n] -= opA[m x k] * opB[n x k]^T
//   a_kmajor = 0: opA(i,kk) = A[i + kk*lda]   (row index contiguous)
//   a_kmajor = 1: opA(i,kk) = A[kk + i*lda]   (k contiguous)          likewise for B.
// tri: 0 = all tiles; 1 = skip tiles entirely above the diagonal, where the diagonal is
//      (global row grow0 + i) == (global col gcol0 + j).
// ktri: 1 = per-tile k range starts at max(tile row0, tile col0) + koff (LAUUM: X^T X with X lower)
struct GemmArgs {
    double* C; int64_t ldc;
    const double* A; int64_t lda; int a_kmajor;
    const double* B; int64_t ldb; int b_kmajor;
    int64_t m, n, k;
    int tri; int64_t grow0, gcol0;
    int ktri;
    int overwrite; // 0: C -= A*B^T; 1: C = +A*B^T (no read of C); 2: C += A*B^T
    int fold_len;  // set by launch_gemm_sub (tri): live tiles per folded tile-column pair
    int total;     // set by launch_gemm_sub: logical workgroups (glds kernel)
    int grid_limit; // set by no caller of the product; tools/gemm_sk.hip reads it (goes with the next change of the kernels' arguments)
    int tile;      // 0: pick by problem size; 128 / 64 / 32: force the 128x128 / 64x64 / 32x64 tile
    int rhs_rows;  // the LAST rhs_rows of the m rows of C / A are right-hand-side rows (engine.hip): the direct-to-LDS
                   // kernels update them with plain FMAs instead of a tile row (gemm_glds64.h: gemm_rhs_rows); inside those
                   // kernels m counts the main rows only
    const int* tile_map; // set by launch_gemm_sub (tri, 128 x 128 direct-to-LDS kernel): workgroup -> tile (ti | tj << 16, or -1: none)
                         // in an order that keeps the operand panels of an XCD's resident workgroups few (gemm.hip: tri_tile_map)
    void* stop_event; // host side only: hipEvent_t completed by this launch (null: none)
    const BatchTab* bt; // batched launch (gridDim.z GPs): set by the launch wrapper, null otherwise
};
static __device__ __forceinline__ void gemm_rebase(GemmArgs& g)
{
    if (g.bt) {
        const int z = (int)blockIdx.z;
        g.C = bt_rebase(g.bt, z, g.C);
        g.A = bt_rebase(g.bt, z, g.A);
        g.B = bt_rebase(g.bt, z, g.B);
    }
}
void launch_gemm_sub(hipStream_t s, const GemmArgs& g);
int debug_tri_tile_map(int64_t m, int64_t n, int64_t grow0, int64_t gcol0, int* out, int cap); // gemm.hip (host only)
// the next-panel update g (as for launch_gemm_sub: C = A[pe:, pe:pe2], k = pe - p0, tri) and, in the same launch, the
// update + factorisation + half-inversion of the next diagonal block A[pe:pe+64, pe:pe+64] (-> Xt_next)
// (Dacc: sum of the pieces the panel steps already formed, subtracted as well; p0 == pe: no products here)
void launch_upd_fused(hipStream_t s, const GemmArgs& g, double* A, int64_t lda, int64_t p0, int64_t pe, double* Xt_next,
                      int* info, const double* Dacc);
double gemm_flops(const GemmArgs& g);

// ---- K^-1 by recursion (inv2.hip): lists of 128 x 128 x k products and of tile folds ------------------------------
// One launch = a LIST of independent tile products C = (+/-) A B^T, A and B contiguous along their non-k index (the operand
// form of k_gemm_glds), each with its own k; persistent workgroups, each with a host-built share of the list (longest first).
// A product whose k range was cut into chunks leaves chunk c > 0 in a partial buffer; a fold list adds them up in fixed
// order (bitwise reproducible) and, where asked, also writes the tile transposed.
struct GemmItem {
    const double* A; // tile row origin at the first k of the chunk: A[r + kk * ld]
    const double* B; // tile column origin likewise: B[c + kk * ld]
    double* C;       // where THIS chunk's product goes (its first mr rows x nc columns: a ragged last tile stores nothing else); never
                     // read by the product: the tile itself for chunk 0 (and for a whole k range), partial buffer c for chunk c > 0
    double* T;       // optional: the finished tile transposed as well, T[c + r * ld] = D[r + c * ld]
    double* D;       // a cut k range: the tile (= chunk 0's C)
    const double* P1; // ... and its place in partial buffer 1 (buffer c: P1 + (c - 1) * pstride)
    int32_t k;       // multiple of 16
    int32_t flags;   // bit 0: the product enters negated; bits 8..15: mr, bits 16..23: nc — valid rows / columns (1 .. tile edge)
    int32_t slot, nch; // nch > 1: one of the nch chunks of a cut k range; `slot` = the tile's counter word.  Every chunk stores its
                     // product write-through and counts; the one that counts LAST adds them up, D + P1 + P2 + .. in that order
                     // whoever it is (bitwise reproducible), stores the tile and its transposed copy: nobody waits for anybody
};
#define GEMM_ITEM_NEG 1
// (batched launches, g_batch: the lists hold member 0's pointers, workgroup z rebases them — dev.h: bt_rebase; member z counts in
// the words z * nslots ..)
void launch_gemm_items(hipStream_t s, const GemmItem* items, const int32_t* bin_start, int nbins, int64_t ld, int tile, int* counters,
                       int nslots, int64_t pstride); // tile: 128 or 64
// the plan of one inversion (inv2.hip): host-built once per (N, ld, buffers), resident on the device
struct Inv2Plan;
Inv2Plan* inv2_plan_get(Inv2Plan* old, int64_t N, int64_t ld, const double* L, double* U, double* Kinv, double* S, int64_t pstride,
                        int members = 1, bool* rebuilt = nullptr); // members: GPs stepped by the launches (a batched sequence: another
                                                                   // plan from four on); rebuilt: the caller zero-fills U and S then
void inv2_plan_free(Inv2Plan* p);
bool inv2_supported(int64_t N);
int inv2_partials();                // N x N partial buffers behind the W / T-form buffer in S (S holds 1 + this many)
double inv2_flops(const Inv2Plan* p); // algorithmic flops of the products (2 N^3 / 3 less the leaves)
void inv2_run(hipStream_t s, Inv2Plan* p, const double* Xt_all, int part = 0); // enqueues the launches (part: inv2.hip)
int inv2_debug_plan(int64_t N, int64_t ld, int nbins, int load_pct, int64_t* out, int64_t cap_rows); // host only (tests)

// ---- vector solves, reductions (solve.hip) -----------------------------------------
// one full triangular sweep over P <= GPE_MAX_P right-hand sides (ceil(N/64) launches):
// trans = 0: out = L^-1 w (top down);  trans = 1: out = L^-T w (bottom up).  w is destroyed.
// Xt_all: inverses of the 64 x 64 diagonal blocks (launch_diag / launch_diag_inv).
void launch_trsv_sweep(hipStream_t s, const double* L, int64_t ld, int64_t N, const double* Xt_all, double* w,
                       double* out, int64_t ldw, int P, int trans);
// the whole backward sweep a = L^-T y in one data-flow launch for nblk = ceil(N/64) <= 256 (the caller
// checks).  y[i * ysi + p * ysp]; err: set to 1 if a hand-off timed out; prefilled: `a` already holds
// the all-ones sentinel; part (optional, 2 nblk doubles): per-block partial sums of log L_ii and
// om . a (part_acc: add to the second half instead of overwriting)
void launch_trsv_bwd_flow(hipStream_t s, const double* L, int64_t ld, int64_t N, const double* Xt_all, const double* y,
                          int64_t ysi, int64_t ysp, double* a, int64_t ldw, int P, int* err, int prefilled, const double* om,
                          int64_t ldom, double* part, int part_acc);
// the same for ONE right-hand side with a_j = g_j - M_j a_{j+1}: the hop is one matrix-vector product (sweep2.hip, round 6)
void launch_trsv_bwd_m(hipStream_t s, const double* L, int64_t ld, int64_t N, const double* Xt_all, const double* y, int64_t ysi, double* a,
                       int* err, int prefilled, const double* om, double* part);
// the whole forward sweep y = L^-1 b in one data-flow launch, nblk <= 256 (the caller checks); b: N x P (ldb),
// y: N x P (ldy), must not alias b; err as above
void launch_trsv_fwd_flow(hipStream_t s, const double* L, int64_t ld, int64_t N, const double* Xt_all, const double* b,
                          int64_t ldb, double* y, int64_t ldy, int P, int* err);
// Arows[p + i*lda] = V[i + p*ldv] (P rows appended under the matrix) and back
void launch_cols_to_rows(hipStream_t s, const double* V, int64_t ldv, int64_t N, int P, double* Arows, int64_t lda,
                         double* sent = nullptr);
void launch_rows_to_cols(hipStream_t s, const double* Arows, int64_t lda, int64_t N, int P, double* V, int64_t ldv);
// out[0] = sum_i log L_ii ; out[1] = sum_{i,p} obs_mean * alpha   (gp.hpp:274-277)
void launch_loglik_terms(hipStream_t s, const double* L, int64_t ldl, int64_t N, const double* om, const double* alpha,
                         int64_t ldv, int P, double* out);
// colsq[m] = sum_i Z[i,m]^2 ; var[m] = kvv[m] - colsq[m]
void launch_col_var(hipStream_t s, const double* Z, int64_t ldz, int64_t N, int64_t M, const double* kvv, double* var);
// kta[m, p] = sum_i Ks[i, m] alpha[i, p]
void launch_kta(hipStream_t s, const double* Ks, int64_t ldk, int64_t N, int64_t M, const double* alpha, int64_t lda,
                int P, double* kta, int64_t ldo);
// the same two for the transposed layout of the batched query path (points contiguous, Zt[m + i ldz]); partial: scratch of
// nseg x (P or 1) x ldp doubles, the segments are added in order (bitwise reproducible)
void launch_row_var_t(hipStream_t s, const double* Zt, int64_t ldz, int64_t N, int64_t M, const double* kvv, double* var,
                      double* partial, int64_t ldp, int nseg);
void launch_kta_t(hipStream_t s, const double* Kst, int64_t ldk, int64_t N, int64_t M, const double* alpha, int64_t lda, int P,
                  double* kta, int64_t ldo, double* partial, int64_t ldp, int nseg);
// misc
void launch_set_identity(hipStream_t s, double* A, int64_t lda, int64_t n);
// inv.hip: Out[o0:o0+pw, o0:o0+pw] = inv(L[o0:o0+pw, o0:o0+pw]) (full square) for every outer panel of nbo <= 256
// columns, from the 64 x 64 block inverses Xt_all
// OutT (optional): the same blocks transposed
void launch_inv_panels(hipStream_t s, const double* L, int64_t ld, int64_t N, int nbo, const double* Xt_all, double* Out,
                       int64_t ldo, double* OutT, int64_t ldt);
// A[0 : rows, 0 : cols] = 0 (column-major, lda) — a kernel, not hipMemsetAsync: it takes part in batched launches
void launch_zero2d(hipStream_t s, double* A, int64_t lda, int64_t rows, int64_t cols);
void launch_symmetrize_from_lower(hipStream_t s, double* A, int64_t lda, int64_t n);
void launch_copy2d(hipStream_t s, const double* src, int64_t lds, double* dst, int64_t ldd, int64_t rows, int64_t cols);
// add_sample tail: L[n,n] = sqrt(knn - ||row||^2)   (gp.hpp:596-597)
void launch_append_diag(hipStream_t s, double* Lrow, int64_t ldl, int64_t n, const double* knn, int* info);

// ---- gradient of the log-likelihood (grad.hpp:285-311) (grad.hip) ------------------
// partial[b, t] per lower-triangle tile b; then a fixed-order final reduction into grad[T]
void launch_grad_loglik(hipStream_t s, const double* Xt, int64_t ldx, int64_t N, const KParams& kp, const double* Kinv,
                        int64_t ldk, const double* alpha, int64_t lda, const double* uvec, int P, int n_theta,
                        int optimize_noise, double* partial, double* grad);
// leave-one-out (gp.hpp:339-402): v = alpha / kappa, sc = sqrt(c), val[i] per-sample terms, out[0] = LOO value
// (v, sc may be null: value only); S = sym(Kl) diag(sc); g[0..n) *= f
void launch_loo_prep(hipStream_t s, const double* Kinv, int64_t ldk, int64_t N, const double* alpha, int64_t lda, int P,
                     double* v, double* sc, double* val, double* out);
void launch_sym_colscale(hipStream_t s, const double* Kl, int64_t ldk, int64_t N, const double* sc, double* S,
                         int64_t lds_);
void launch_scale_vec(hipStream_t s, double* g, int n, double f);
int64_t grad_partial_size(int64_t N, int T);

// ---- one-launch small-N path (small.hip): add_sample and point queries below ~256 samples ------------
struct SmallAddArgs {
    double* A;          // factor (and, on exit, its new row n)
    int64_t ld;
    double* Xinv;
    double* Xt;         // SoA samples, column n is written
    int64_t ldx;
    double* Om;         // device obs_mean (ld), rewritten
    double* Al;         // device alpha (ld), rewritten
    const double* om_host; // pinned: (n + 1) x P, column-major, ld = n + 1
    double* out;        // pinned: [0] sum log L_ii, [1] sum obs_mean . alpha
    int* info;          // pinned: first non-positive pivot (1-based), written if zero
    unsigned long long* seq; // pinned: sequence word, written last
    unsigned long long seq_val;
    int n;              // samples before this call = index of the new one
};
struct SmallQueryArgs {
    const double* L;
    int64_t ld;
    const double* Xinv;
    const double* Xt;
    int64_t ldx;
    const double* Al;
    int P, n, M, D;
    const double* xq_host;  // pinned: M x D row-major query points
    double* kta_host;       // pinned: M x P, column-major (ld = M), may be null
    double* var_host;       // pinned: M, may be null
    unsigned long long* seq; // pinned: M sequence words (one per point)
    unsigned long long seq_val;
    int want_kta, want_var;
};

struct SmallAlphaArgs {
    const double* L;
    int64_t ld;
    const double* Xinv;
    const double* om_src; // obs_mean to solve for: pinned host memory (ldom = n) or the device copy (ldom = ld)
    int64_t ldom;
    double* Om;           // device obs_mean to refresh (null: om_src IS the device copy)
    double* Al;
    double* out;          // pinned: [0] sum log L_ii, [1] sum obs_mean . alpha
    unsigned long long* seq;
    unsigned long long seq_val;
    int n;
};
int small_max_n();
void launch_small_alpha(hipStream_t s, const SmallAlphaArgs& g, int P);
void launch_small_add(hipStream_t s, const SmallAddArgs& g, int P, const KParams& kp, const LamParams& lp, const double* x);
void launch_small_query(hipStream_t s, const SmallQueryArgs& g, const KParams& kp, const LamParams& lp);

// ---- joint posterior over a point batch (joint.hip; include/gpe_joint.h) ------------------------------------------
// the split of Sigma's product Zt Zt^T (k = N) over workgroups: chunks per tile, and the launch's (tile i, tile j, k0, k1, slot) rows
int joint_cov_chunks(int64_t M, int64_t N, int cus);
int joint_cov_plan(int64_t M, int64_t N, int cus, int64_t* out, int64_t cap_rows); // host only
// Sig (full symmetric, lds) = k(V, V) + jitter I - sum_c Part_c, the partial matrices (ldp, pstride apart) added in ascending c
void launch_cov_fold(hipStream_t s, const double* Part, int64_t ldp, int64_t pstride, int nch, const double* Qt, int64_t ldq, int64_t M,
                     const KParams& kp, double jitter, double* Sig, int64_t lds);
// F[m + M col] = mean_q[m + M p] + kta[m + ldk p] + sum_{j <= m} C[m, j] Z[j + M col], col = s + S p < ncols (mean_q may be null)
void launch_draws(hipStream_t s, const double* Cm, int64_t ldc, int64_t M, const double* Z, const double* mean_q, const double* kta, int64_t ldk,
                  int S, int ncols, double* F);
// out[2 col] = max of column col of F, out[2 col + 1] = the bits of the lowest index (int64) that holds it
void launch_argmax(hipStream_t s, const double* F, int64_t M, int ncols, double* out);

// ---- greedy batch selection with hallucinated observations (select.hip; include/gpe_batch_select.h) --------------------
#define SEL_RULE_UCB 0
#define SEL_RULE_EI 1
#define SEL_RULE_VAR 2
// the words the rounds hand on from launch to launch (device memory, zeroed before the first launch)
struct SelState {
    long long j;    // this round's pick
    long long fail; // 0, or the status of the call: the 1-based round whose pivot was not positive; every later launch returns at once
    long long bad;  // set by k_sel_fold of a round with such a pivot, turned into `fail` by the launch behind it
};
int select_chunks(int64_t M, int64_t N, int cus);
int select_fold_groups(int64_t M); // workgroups of the fold = (value, index) pairs a round leaves
int select_plan(int64_t M, int64_t N, int cus, int64_t* out, int64_t cap_rows); // host only: gpe_debug_select_plan
struct SelRound {
    SelState* st;
    const int64_t* plan; // device copy of select_plan's rows
    int64_t nrows;
    int nch;
    const double* Zt; // Zt[m + i ldz], i < N
    int64_t ldz, N, M;
    const double* Qt; // the candidates, SoA
    int64_t ldq;
    const KParams* kp; // host copy
    double *zj, *wj;   // row j of Zt (N) and of W (q)
    double* part;      // nch partial vectors, ldp apart
    int64_t ldp;
    double* W; // M x q
    int64_t ldw;
    double* var;      // var_t, updated in place
    const double* mu; // M
    int* picked;      // M, zeroed
    double* pairs;    // 2 per workgroup of the fold
    long long* idx;   // q
    double* score;    // q
    int q, rule, distinct;
    double param, var_add, obs_noise;
};
// Zt[m + i ldz] = Z[i + m ld] (the N x M layout of the small models, once per call)
void launch_sel_transpose(hipStream_t s, const double* Z, int64_t ld, int64_t N, int64_t M, double* Zt, int64_t ldz);
void launch_sel_score0(hipStream_t s, const SelRound& g);      // the scores of round 0 and its pick
void launch_sel_round(hipStream_t s, const SelRound& g, int t); // round t: gather, column product, fold, the pick of round t + 1

// ---- the knowledge gradient over a finite alternative set (kg.hip; include/gpe_kg.h) --------------------------------------
// kg[m] = h(a, b_m) for m < M, one workgroup each.  var == null: column m of B (A x M, ldb) holds the slopes.  Otherwise B is the
// unscaled covariance and b = B[:, m] / sqrt(var[m] + obs_noise) — kg[m] = 0 where that sum is not above DBL_EPSILON or not
// finite — and, with_self, the candidate itself is line A: (mu_c[m], var[m] / sqrt(var[m] + obs_noise)).  nseg (may be null): the
// steps of the chain.  A <= GPE_KG_MAX_ALTERNATIVES (the lines, their breakpoints and successors are in LDS).
void launch_kg_envelope(hipStream_t s, const double* a, int A, const double* B, int64_t ldb, int64_t M, const double* var, double obs_noise,
                        int with_self, const double* mu_c, double* kg, int* nseg);

// ---- the marginal beliefs of an acquisition's candidates (belief.h; ehvi.hip, cei.hip, mes.hip) ---------------------------
// Belief j of candidate m: the mean mu[m + col[j] ldmu] (+ add[m + j lda]; add == null: nothing is added); var == null: the standard
// deviation sd[m + j lds]; otherwise one model's outputs share sqrt((var[m] > DBL_EPSILON ? var[m] : 0) + var_add).  mu_out (may be
// null): the means as used, column j at mu_out + j ldm.
constexpr int BELIEF_MAX = 17; // GPE_CEI_MAX_CONSTRAINTS + 1 (acq.hpp holds it to that)
struct BeliefArgs {
    const double *mu, *add, *sd, *var;
    int64_t ldmu, lda, lds;
    double var_add;
    int col[BELIEF_MAX];
    double* mu_out;
    int64_t ldm;
};

// ---- the two-objective expected hypervolume improvement (ehvi.hip; include/gpe_ehvi.h) ----------------------------------
// ehvi[m] and, partials != null, the four partials (column c at partials + c ldp) of candidate m < M over the prepared front
// (device, row-major n x 2, n <= GPE_EHVI_MAX_FRONT: it sits in LDS) and (r1, r2); one wave each.  Beliefs 0 and 1 of b: the objectives.
struct EhviArgs {
    const double* front;
    int n;
    double r1, r2;
    BeliefArgs b;
    int64_t M;
    double *ehvi, *partials;
    int64_t ldp;
};
void launch_ehvi2(hipStream_t s, const EhviArgs& q);

// ---- the three-objective expected hypervolume improvement (ehvi3.hip; include/gpe_ehvi3.h) ------------------------------
// ehvi[m] and, ntab == 3, the six partials (column c at partials + c ldp) of candidate m < M; one wave each.  tables (device): ntab
// box tables one behind the other, rows {l_a, u_a, l_b, u_b, h}, nb[t] rows each; table 0: height axis 2 (the value and the partials
// of objective 3), tables 1 and 2 (ntab == 3): height axes 0 and 1.  Beliefs 0 .. 2 of b: the objectives.
struct Ehvi3Args {
    const double* tables;
    int ntab, nb[3];
    BeliefArgs b;
    int64_t M;
    double *ehvi, *partials;
    int64_t ldp;
};
void launch_ehvi3(hipStream_t s, const Ehvi3Args& q);

// ---- constrained expected improvement in the log domain (cei.hip; include/gpe_cei.h) ------------------------------------
// logcei[m] and, where asked, terms (column j at terms + j ldt, j <= C) and partials (column j at partials + j ldp, j < 2 + 2 C) of
// candidate m < M; one thread each.  Belief 0 of b: the objective (with_ei == 0: not read), 1 .. C: the constraints.
struct CeiArgs {
    int with_ei, C;
    double f_best, xi;
    double thr[16]; // GPE_CEI_MAX_CONSTRAINTS
    BeliefArgs b;
    int64_t M;
    double *logcei, *terms, *partials;
    int64_t ldt, ldp;
};
void launch_logcei(hipStream_t s, const CeiArgs& q);

// ---- max-value entropy search in the log domain (mes.hip; include/gpe_mes.h) --------------------------------------------
// logmes[m] and, where asked, terms (column j at terms + j ldt, j < J) and partials (d/d mu_j at partials + j ldp, d/d s_j at
// partials + (J + j) ldp) of candidate m < M; one wave each.  ystar: K x J column-major on the device, finite.  Beliefs 0 .. J - 1 of
// b: the outputs (J <= GPE_MES_MAX_OUTPUTS).
struct MesArgs {
    int J, K;
    const double* ystar;
    BeliefArgs b;
    int64_t M;
    double *logmes, *terms, *partials;
    int64_t ldt, ldp;
};
void launch_mes(hipStream_t s, const MesArgs& q);

// ---- noisy expected improvement in the log domain (nei.hip; include/gpe_nei.h) -------------------------------------------
// lognei[m] and, terms != null, the S terms (terms[s + m ldt]) of candidate m < M; one wave each.  fplus: the S incumbents, on the
// device; cmean[s + m ldm]: the mean at candidate m given draw s.  cvar == null: the standard deviation csd[m]; otherwise
// sqrt(cvar[m] > DBL_EPSILON ? cvar[m] : 0) (belief.h's clamp).  S <= GPE_NEI_MAX_SAMPLES.
struct NeiArgs {
    int S;
    const double* fplus;
    double xi;
    const double* cmean;
    int64_t ldm;
    const double *csd, *cvar;
    int64_t M;
    double *lognei, *terms;
    int64_t ldt;
};
void launch_lognei(hipStream_t s, const NeiArgs& q);
// fplus[s] = max_i F[i + B s], s < S
void launch_nei_colmax(hipStream_t s, const double* F, int64_t B, int S, double* fplus);
// per candidate m < M, from column m of U (B x M, ldu): cvar[m] = var[m] - |U[:, m]|^2, mu_out[m] = kta[m] (+ add[m]; add == null:
// nothing is added), cmean[s + m ldm] = mu_out[m] for s < S
void launch_nei_cond(hipStream_t s, const double* U, int64_t ldu, int64_t B, const double* kta, const double* add, const double* var, int64_t M,
                     int S, double* mu_out, double* cvar, double* cmean, int64_t ldm);

// ---- posterior draws as functions of the query point (pathwise.hip; include/gpe_pathwise.h) -----------------------------
// slots per (segment, column) of a pass's partial sums: the value and, grad, one per row of a point
int paths_slots(bool grad, int R);
// one pass over NB basis functions for M points: mode 0 the Fourier features (Bt = Omega0 by rows, Cf = amp W), mode 1 the data term
// (Bt = the samples by rows, scaled: launch_paths_scale_rows; Cf = U);  part[((seg ncol + c) slots + slot) ldp + m]
void launch_paths_basis(hipStream_t s, int mode, bool grad, const double* Qt, int64_t ldq, int64_t M, const double* Bt, int64_t ldb, int64_t NB,
                        const double* phase, const double* Cf, int64_t ldc, int ncol, const KParams& kp, int nseg, double* part, int64_t ldp);
void launch_paths_scale_rows(hipStream_t s, const double* src, int64_t lds, double* dst, int64_t ldd, int64_t n, const KParams& kp);
void launch_paths_fold(hipStream_t s, const double* partF, int nsegF, const double* partK, int nsegK, int64_t ldp, int NS, int ncol, int64_t M,
                       const KParams& kp, const LamParams& lp, const double* mean, int64_t ldm, int S, double* F, int64_t ldf, double* dF,
                       int64_t ldo);
void launch_paths_residual(hipStream_t s, const double* partF, int nsegF, int64_t ldp, int ncol, int64_t n, int64_t i0, const double* om,
                           int64_t ldom, int S, int c_first, const double* E, int64_t lde, double sn, double* Rt, int64_t ldr);
void launch_paths_untranspose(hipStream_t s, const double* Wt, int64_t ldw, int64_t n, int ncol, double* U, int64_t ldu);
void launch_paths_argmax(hipStream_t s, const double* F, int64_t ldf, int64_t M, int ncol, int64_t t0, bool first, double* run);

// ---- gradient of the batched posterior in the query point (qgrad.hip; include/gpe_query_grad.h) ------------------------
size_t query_grad_partial_doubles(int nseg, int ncol, int R, int64_t ldp);
// columns [cbeg, cbeg + ncol) of { alpha_0 .. alpha_{P-1}, -2 Wt } (Wt = (K^-1 k(X, V))^T, M x N, ldw; null unless column P is among
// them): out[m + ldo (d + Din c)] = sum_i C_c[m, i] d k(v_m, x_i) / d v_d, c counted from cbeg.  The samples are cut into nseg
// segments whose partials (part: query_grad_partial_doubles) are added in ascending order — no floating-point atomics.
void launch_query_grad(hipStream_t s, const double* Qt, int64_t ldq, int64_t M, const double* Xt, int64_t ldx, int64_t N, const double* Wt,
                       int64_t ldw, const double* Al, int64_t lda, int P, const KParams& kp, const LamParams& lp, int cbeg, int ncol, int nseg,
                       double* part, int64_t ldp, double* out, int64_t ldo);

// ---- blocked append of a sample batch (append.hip; include/gpe_append.h) -------------------------------------------
int append_max_chunk(); // rows the tail factorises at once
void append_slices(int64_t n, int64_t* kslice, int* nsl); // the split of the k range (length n) of one chunk's product over workgroups
int append_slices_cap(int64_t n);          // >= the slice count of every order <= n
size_t append_scratch_doubles(int64_t n);  // scratch of launch_append_tail for a call whose chunks see orders <= n: (cap + 1) matrices
// q <= append_max_chunk() new rows of the factor A (order n, ld): A[n + a, k] = Zt[a + k ldq] (k < n) and, at (n, n),
// C = chol(k(V, V) + diag_add I - Zt Zt^T) with V = the SoA points Qt (ldq).  The k range is split over workgroups and folded in
// a fixed order; info: first non-positive pivot (n + j + 1), written only if still 0.  The caller refreshes the block inverses.
// scratch holds slices_cap partial matrices, then S; false (nothing launched) if this order needs more slices than that.
bool launch_append_tail(hipStream_t s, const double* Zt, const double* Qt, int64_t ldq, int q, int64_t n, const KParams& kp, double* A,
                        int64_t ld, int* info, double* scratch, int slices_cap);

// ---- removal of samples by a blocked factor update (remove.hip; include/gpe_remove.h) ------------------------------
#define GPE_RM_CAP 32   // update vectors carried per pass (gpe_remove_max_vectors)
#define GPE_RM_PANEL 256 // columns of the old factor per rot / apply launch pair
// the indices one pass removes from its source factor, ascending; vector k is born at column idx[k]
struct RmList {
    int a;
    int idx[GPE_RM_CAP];
};
int remove_max_vectors();
// scratch of one call on a factor of order n: U (n rounded up to 64, x GPE_RM_CAP), the coefficient table of one panel and the
// kept samples' old indices (int32)
size_t remove_u_ld(int64_t n);
size_t remove_coef_doubles();
// Xt[j + d ld] <- Xt[keep[j] + d ld] for j < n_new, 0 for n_new <= j < n_old, in place, every one of `rows` rows
void launch_rm_xt(hipStream_t s, double* Xt, int64_t ld, int rows, const int* keep, int64_t n_new, int64_t n_old);
// columns [0, ch) of the old factor (none of them removed): the kept rows move up
void launch_rm_head(hipStream_t s, const double* src, double* dst, int64_t ld, int64_t n, int64_t ch, const RmList& R);
// the panel of old columns [c0, min(c0 + GPE_RM_PANEL, n)): k_rm_rot on its triangle rows (reflectors into coef, finished rows to
// dst), then k_rm_apply on every row below (none for the last panel).  first: no vector is older than this panel (U is not read).
// Returns the number of launches
int launch_rm_panel(hipStream_t s, const double* src, double* dst, int64_t ld, int64_t n, int64_t c0, const RmList& R, bool first, double* U,
                    int64_t ldu, double* coef);

// ---- sparse pseudo-input GP (sparse.hip; include/gpe_sparse.h) -----------------------------------------------------
// V (M pseudo-inputs x a chunk of nc points) in either layout of the batched query: element (n, i) at Z[n sn + i si]
int64_t sparse_default_chunk(int64_t M);             // columns of V per chunk unless GPE_SPARSE_CHUNK says otherwise
int sparse_gram_slices(int64_t M, int64_t len, int cus); // slices the k range of a chunk of len columns is cut into
int64_t sparse_gram_plan(int64_t M, int64_t N, int64_t chunk, int cus, int64_t* out, int64_t cap_rows); // host only: gpe_debug_gram_plan
// ep[n] = 1 + (c - sum_i Z[n, i]^2) / sig, w[n] = 1 / ep[n]   (spgp.hpp:399)
void launch_sp_ep(hipStream_t s, const double* Z, int64_t sn, int64_t si, int64_t nc, int64_t M, double c, double sig, double* ep, double* w);
// R[i + p ldr] += sum_n Z[n, i] w[n] y[n + p ldy]
void launch_sp_r(hipStream_t s, const double* Z, int64_t sn, int64_t si, int64_t nc, int64_t M, const double* w, const double* y, int64_t ldy,
                 int P, double* R, int64_t ldr);
// out[0] = sum log ep, out[1 + p] = sum_n y[n, p]^2 / ep[n]
void launch_sp_sums(hipStream_t s, const double* ep, int64_t N, const double* y, int64_t ldy, int P, double* out);
void launch_sp_scale(hipStream_t s, const double* Z, int64_t sn, int64_t si, int64_t nc, int64_t M, const double* w, double* Zw);
// one workgroup per plan row (device copy of sparse_gram_plan's rows of this chunk; n0 / slot0: the chunk's first column / slot).
// mode 0: partial tiles into Out + (slot - slot0) pstride; 1: A's tiles = the product; 2: += (one slice per tile only)
void launch_sp_gram(hipStream_t s, const double* Z, int64_t sn, int64_t si, const double* w, int64_t n0, int64_t M, const int64_t* plan,
                    int64_t rows, int64_t slot0, double* Out, int64_t ldo, int64_t pstride, int mode);
void launch_sp_fold(hipStream_t s, const double* Part, int64_t ldp, int64_t pstride, int nsl, int first, int64_t M, double* A, int64_t lda);
void launch_sp_diag_add(hipStream_t s, double* A, int64_t lda, int64_t M, double v);
void launch_sp_s2(hipStream_t s, const double* v1, const double* v2, double sig, int64_t T, double* s2);

// ---- the sparse GP's analytic gradient (sparse_grad.hip; include/gpe_sparse_grad.h) ------------------------------------
// a chunk in the transposed layout: Kt[n + j ldq] = K~_jn, ILVt = V~t Lm^-T, B1t = ILVt Lt^-1, IQt = V~t L^-1
int64_t sparse_grad_default_chunk(int64_t M);                // points per chunk: four M x chunk buffers are live
int sparse_grad_row_slices(int64_t M, int64_t len, int cus); // slices of a chunk's points in k_sp_grow
// b1 = Lti^T bet (Lti lower, order M): b1[j + p ldo]
void launch_sp_gb1(hipStream_t s, const double* Lti, int64_t ld, int64_t M, const double* bet, int64_t ldb, int P, double* b1, int64_t ldo);
void launch_sp_grs(hipStream_t s, const double* ep, int64_t nc, double* rs); // rs = 1 / sqrt(ep)
// per point, from ILVt = (Lm^-1 V~)^T and IQt: big = bigsum, R[n + p ldq] = (y~ - mu) / sig; part[3 workgroup + {0, 1, 2}] = shares of
// S_sig, S_epc, S_mu
void launch_sp_gcol(hipStream_t s, const double* ILVt, const double* IQt, int64_t ldq, int64_t nc, int64_t M, const double* bet, int64_t ldbet, int P,
                    const double* y, int64_t ldy, const double* ep, const double* rs, double c, double sig, double dl, double* big, double* R,
                    double* part);
// Vst[n + i ldq] = rs[n] Z[n sn + i si] (V of the chunk in either layout -> scaled, transposed); T = A^T (order M, both ld)
void launch_sp_gvt(hipStream_t s, const double* Z, int64_t sn, int64_t si, int64_t nc, int64_t M, const double* rs, double* Vst, int64_t ldq);
void launch_sp_gtrans(hipStream_t s, const double* A, double* T, int64_t ld, int64_t M);
// Racc[j + col ldp] (=, first) or (+=) sum_n G_jn [1, x^, x^2]_n,col over the chunk, S slices folded in ascending order; Part: S x
// (2 D + 1) x ldp doubles of scratch; Qt: the chunk's SoA coordinates (ldq)
void launch_sp_grow(hipStream_t s, const double* Kt, const double* B1t, const double* IQt, int64_t ldq, int64_t nc, int64_t M, const double* b1,
                    int64_t ldb1, int P, const double* big, const double* R, const double* Qt, const KParams& kp, double sig, int S, double* Part,
                    int64_t ldp, int first, double* Racc);
// dxb (M x D row-major), dhp (D + 2) from the M x M matrices (symmetric, ldm), Racc and the nblk per-workgroup scalar shares
void launch_sp_gfinish(hipStream_t s, const double* Xt, int64_t ldx, const KParams& kp, int64_t M, int P, const double* b1, int64_t ldb1,
                       const double* IQm, const double* IAm, const double* TT, int64_t ldm, const double* Racc, double sig, double dl,
                       const double* part, int64_t nblk, double* dxb, double* tb, double* cs, double* dhp);

// ---- micro-benchmarks (microbench.hip) ---------------------------------------------
double run_mfma_f64_peak(hipStream_t s);
double run_hbm_stream_peak(hipStream_t s);
