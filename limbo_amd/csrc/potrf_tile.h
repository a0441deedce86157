// potrf_tile.h — what potrf.hip, potrf_panel.hip and potrf_tail.hip share, included by nothing else: the tile constants, the products
// over [kk][i] operand tiles, the lane = row form of an accumulator tile, the polled hand-over.  A helper of ONE family lives in its file.
#pragma once
#include "dev.h"
#include <atomic>
#include <cstdio>

#define NB 64
#define XS 66 // LDS row stride (doubles) of the 64 x 64 work matrices: conflict-free MFMA operand reads

#include "gemm_glds64.h" // mfma4, and the 64 x 64 GEMM body for the fused next-panel update

static __device__ __forceinline__ double bcast_lane(double v, int src)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

#define DIAG_LTB (4 * NB * 4) // LDS doubles of the four round buffers of DiagRound (potrf.hip); diag_flow.h carves its H out of them
#include "diag_flow.h"
#include "kfun_fast.h"
#define DIAG_THREADS 512
// the data-flow block alone: defined in potrf_panel.hip (k_panel_step's workgroup 0 runs the same code), launched by launch_diag (potrf.hip)
__global__ void k_diag(double* A, int64_t lda, double* Xt, int* info, int64_t goff);
__global__ void k_diag_b(double* A, int64_t lda, double* Xt, int* info, int64_t goff, const BatchTab* bt);

#define PS 80 // stride (doubles) of the [kk][i] operand tiles: == 16 mod 32

// acc[m][n] += sum_{k in [k0, k0+KLEN)} Aop[k][wm + 16 m + ..] * B(col, k)  — 8 waves.
//   wave tile: 32 rows x (4 RBN) columns starting at column wn
//   BKM = true : B stored k-contiguous, B(col, k) = Bop[col * XS + k]     (X or L blocks, [c][k])
//   BKM = false: B stored [kk][n],      B(col, k) = Bop[k * PS + col]
template <bool BKM, int KLEN, int RBN, int BS = XS> // BS: row stride of a k-contiguous B
static __device__ __forceinline__ void mmk(const double* __restrict__ Aop, int ak0, const double* __restrict__ Bop,
                                           int bk0, int wm, int wn, int lane, double (&acc)[2][RBN])
{
    const int ar = wm + (lane & 15), bc = wn + (lane & 3), kq = lane >> 4;
#pragma unroll
    for (int ks = 0; ks < KLEN; ks += 4) {
        double af[2], bf[RBN];
#pragma unroll
        for (int x = 0; x < 2; ++x)
            af[x] = Aop[(ak0 + ks + kq) * PS + ar + 16 * x];
#pragma unroll
        for (int x = 0; x < RBN; ++x)
            bf[x] = BKM ? Bop[(bc + 4 * x) * BS + bk0 + ks + kq] : Bop[(bk0 + ks + kq) * PS + bc + 4 * x];
#pragma unroll
        for (int n = 0; n < RBN; ++n)
#pragma unroll
            for (int m = 0; m < 2; ++m)
                acc[m][n] = mfma4(af[m], bf[n], acc[m][n]);
    }
}
template <bool BKM>
static __device__ __forceinline__ void mm64(const double* __restrict__ Aop, const double* __restrict__ Bop, int wm, int wn,
                                            int lane, double (&acc)[2][4])
{
    mmk<BKM, NB, 4>(Aop, 0, Bop, 0, wm, wn, lane, acc);
}

// The 32 x 16 accumulator tile of one wave of k_panel_step (acc[m][n]: v_mfma_f64_4x4x4 layout, lane l on
// row 16 m + 4*((l>>2)&3) + (l>>4), column 4 n + (l&3)) re-arranged with cross-lane moves into the
// lane = row layout used for all C traffic: out[it] = element (row = lane & 31, column 2 it + (lane >> 5)).
// A global load/store in the MFMA layout touches 4 columns x 16 rows with neighbouring lanes in
// different columns and costs ~150 (load) / ~450 (store) cycles just to issue (gemm.hip, WaveTileC);
// in the row layout an instruction covers two whole 256-byte column pieces.
static __device__ __forceinline__ void wave_tile_to_rows(const double (&acc)[2][4], double (&out)[8], int lane)
{
    const int row = lane & 31;
    const int src_base = 16 * (row & 3) + 4 * ((row >> 2) & 3);
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int src = src_base + ((2 * it + (lane >> 5)) & 3);
        const double v0 = __shfl(acc[0][it >> 1], src);
        const double v1 = __shfl(acc[1][it >> 1], src);
        out[it] = (row >> 4) ? v1 : v0;
    }
}

struct P256 {
    double* A;
    int64_t lda, p0, R0;
    double* Xt;
    int* info;
    int spin_limit, nrows;
    bool mute, want_d;
    double *Bx, *T0, *T1, *T2;
    double* S22; // the polled copies of X11 | L21 | X22 of diagonal blocks 1..3 (3 x 3 x 1024 doubles), armed by the launch before
    double* HP;  // ... and of the six head tiles (P256_H), 4096 doubles each: they travel the same way, no flag, no acknowledgement
};

// Waiting for a polled block costs memory traffic: 60 strips x 512 threads each re-reading their 2..8 words every microsecond
// is 10^5 uncached transactions per look — it slows everybody's loads (measured: 1.452 -> 1.436 ms per evaluation without it).
// So a wave first watches ONE word of the block, the same for all its lanes (one transaction per look, with a pause), chosen
// among the last to be written, and only then fetches and checks its own.
static __device__ __forceinline__ void poll_one(const double* p, int spin_limit, int* __restrict__ info)
{
    const unsigned long long* w = reinterpret_cast<const unsigned long long*>(p);
    int spins = 0;
    while (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ~0ull) {
        if (++spins > spin_limit) {
            if ((threadIdx.x & 63) == 0)
                info[2] = 1;
            break;
        }
        __builtin_amdgcn_s_sleep(2);
    }
    asm volatile("" ::: "memory");
}

// a 64 x 64 tile (ld 64) that another workgroup of this launch is writing, or has written, over an all-ones pattern:
// thread t holds elements (t & 63, (t >> 6) + 8 q) as in TileRegs
// Round 4: the FIRST look at a polled block is an ordinary (cacheable) load, only the re-reads of words that still showed the
// pattern are device-scope.  A device-scope load is served by the memory side, whatever the XCD's L2 holds: every one of the
// nb - s workgroups that use an L tile fetched its 32 KB over the fabric — 2.8 GB per batch of eight N = 2048 factorisations,
// 0.85 GB in the tall launch of N = 4096, both at the ~2 TB/s such loads reach (round-4 measurement: eight interleaved
// factorisations took 3.3x one).  The protocol makes the cached look safe: inside a launch a slot only ever changes from the
// pattern to its final value, word by word (the launch before armed it, and kernel boundaries write back / invalidate the
// L2s), so whatever a cache line holds, a word that is not the pattern is final; a word that is goes the device-scope way.
#define POLL_FIRST_SCOPE __HIP_MEMORY_SCOPE_WORKGROUP
struct PolledTile {
    unsigned long long b[8];
    __device__ __forceinline__ void issue(const double* G)
    {
        const unsigned long long* g = reinterpret_cast<const unsigned long long*>(G) + (threadIdx.x & 63) + (threadIdx.x >> 6) * NB;
#pragma unroll
        for (int q = 0; q < 8; ++q)
            b[q] = __hip_atomic_load(g + 8 * q * NB, __ATOMIC_RELAXED, POLL_FIRST_SCOPE);
    }
    __device__ __forceinline__ void finish(const double* G, int spin_limit, int* __restrict__ info)
    {
        const unsigned long long SENT = ~0ull;
        const unsigned long long* g = reinterpret_cast<const unsigned long long*>(G) + (threadIdx.x & 63) + (threadIdx.x >> 6) * NB;
        int spins = 0;
        while (b[0] == SENT || b[1] == SENT || b[2] == SENT || b[3] == SENT || b[4] == SENT || b[5] == SENT || b[6] == SENT
               || b[7] == SENT) {
            if (++spins > spin_limit) {
                info[2] = 1;
                break;
            }
            poll_one(G + NB * NB - 1, spin_limit, info);
            if (b[0] == SENT) b[0] = __hip_atomic_load(g + 0 * NB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (b[1] == SENT) b[1] = __hip_atomic_load(g + 8 * NB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (b[2] == SENT) b[2] = __hip_atomic_load(g + 16 * NB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (b[3] == SENT) b[3] = __hip_atomic_load(g + 24 * NB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (b[4] == SENT) b[4] = __hip_atomic_load(g + 32 * NB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (b[5] == SENT) b[5] = __hip_atomic_load(g + 40 * NB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (b[6] == SENT) b[6] = __hip_atomic_load(g + 48 * NB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (b[7] == SENT) b[7] = __hip_atomic_load(g + 56 * NB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __device__ __forceinline__ void store(double* __restrict__ T) const
    {
        const int i = threadIdx.x & 63, kk0 = threadIdx.x >> 6;
#pragma unroll
        for (int q = 0; q < 8; ++q)
            T[(kk0 + 8 * q) * PS + i] = __longlong_as_double((long long)b[q]);
    }
};

// the bound of the polls inside a launch; test hook GPE_HANDOVER_FAULT: negative = nobody publishes, every hand-over "times out" at once
static inline int flow_spin_limit()
{
    static const bool fault = env_flag("GPE_HANDOVER_FAULT", false);
    return fault ? -16 : GPE_FLOW_SPIN_LIMIT;
}
