// shell_layout.h — the layout of a handle's shell, stated once.  No HIP in here (tests/cpp/test_shell_layout.cpp).
// The shell (engine.hip: Shell) is what survives a handle: two streams, ONE device block [scalars | head block] and ONE coherent
// pinned block [info words | sequence words | hScal | hSmall].  Every region of the two blocks and every slot a caller indexes
// has its name here, in doubles unless it says bytes; the accessors take the block's base.  What keeps two regions apart is a
// static_assert below, not the way the numbers happen to fall: a change that moves or adds a region finds its neighbours there.
#pragma once
#include <stddef.h>

#define GPE_MAX_P 8 // outputs handled per solve launch (and per point of the small path's query: the kta slots below)

namespace shell {
constexpr int EDGE = 64, PANEL = 256; // NB and NBO of the host side and the kernels (asserted where those are defined)
constexpr int TILE = EDGE * EDGE;     // doubles of one tile
} // namespace shell

// k_panel256's polled hand-over buffer (potrf_panel.hip), one per S22 region below
#define P256_POLLED_S (9 * 1024)                             // X11 | L21 | X22 of three diagonal blocks
#define P256_POLLED_DOUBLES (P256_POLLED_S + 6 * shell::TILE) // ... and six head tiles: 33,792 doubles per buffer

namespace shell {

// ---- the device block: [scalars SCAL_DOUBLES | head block HEAD_TILES tiles] --------------------------------------------------
constexpr int SCAL_DOUBLES = 1024;
constexpr int SCAL_LOGDET = 0, SCAL_TRACE = 1, SCAL_KNN = 2; // sum log L_ii, trace(om^T alpha) (k_loglik_terms), k_knn's scratch
// The head block: two halves of HALF_TILES tiles, chosen by panel parity, then two single tiles.  Of a half:
//   [0, STEP_HEAD_TILES)               the head tiles of the step-by-step panel (k_panel_step), 3 + 2 + 1 of a 256-column panel
//   [S22_TILE, S22_TILE + S22_TILES)   a polled hand-over buffer of k_panel256 (P256_POLLED_DOUBLES, all-ones when armed)
constexpr int HALF_TILES = 32;
constexpr int STEP_HEAD_TILES = (PANEL / EDGE) * (PANEL / EDGE - 1) / 2;
constexpr int S22_TILE = 20, S22_TILES = 9;
constexpr int DIAG_SUM_TILE = 2 * HALF_TILES; // the scratch sum of the next panel's first diagonal block (k_upd_fused)
constexpr int FLAG_TILE = DIAG_SUM_TILE + 1;  // hand-over flag words, one per head tile, indexed parity * HALF_TILES + head tile
constexpr int HEAD_TILES = FLAG_TILE + 1;
constexpr size_t HEAD_BYTES = sizeof(double) * HEAD_TILES * TILE;
constexpr size_t DEV_BYTES = sizeof(double) * SCAL_DOUBLES + HEAD_BYTES;
typedef unsigned long long flag_t; // (dev.h: gpe_epoch_t)

inline double* head(double* dev) { return dev + SCAL_DOUBLES; }
inline double* head_half(double* dev, int parity) { return head(dev) + (size_t)parity * HALF_TILES * TILE; }
inline double* s22(double* dev, int parity) { return head_half(dev, parity) + S22_TILE * TILE; }
inline double* diag_sum(double* dev) { return head(dev) + DIAG_SUM_TILE * TILE; }
inline flag_t* flag_tile(double* dev) { return (flag_t*)(head(dev) + FLAG_TILE * TILE); }
inline flag_t* hflags(double* dev, int parity) { return flag_tile(dev) + parity * HALF_TILES; }

static_assert(STEP_HEAD_TILES <= S22_TILE, "the stepped panel's head tiles end at or below the polled buffer");
static_assert(S22_TILE + S22_TILES <= HALF_TILES, "the polled buffer ends inside its half");
static_assert(P256_POLLED_DOUBLES <= S22_TILES * TILE, "k_panel256's polled buffer fits its tiles");
static_assert(2 * HALF_TILES * sizeof(flag_t) <= sizeof(double) * TILE, "a flag word per head tile of both halves fits the flag tile");
static_assert(SCAL_KNN < SCAL_DOUBLES && DEV_BYTES == 8192 + 66 * 4096 * 8, "the device block: 2,170,880 bytes");

// ---- the pinned block: [info words | sequence words | hScal | hSmall], byte offsets ---------------------------------------------
constexpr size_t INFO_BYTES = 64;            // int words the kernels write directly (gpe_ctx::hInfo: pivot, hand-off, hand-over)
constexpr size_t SEQ_OFF = INFO_BYTES;       // the words the small path's host side spins on
constexpr int SEQ_WORDS = 8;                 // ... one per query point (word 0 for add_sample, update_alpha)
constexpr size_t HSCAL_OFF = SEQ_OFF + 64;   // (what gpe_create zeroes lies in front of it)
constexpr int HSCAL_DOUBLES = 1024;
constexpr size_t HSCAL_BYTES = sizeof(double) * HSCAL_DOUBLES;
// hScal: [0], [1] the two log-likelihood terms (as SCAL_LOGDET, SCAL_TRACE), then the backward sweep's per-block partials:
// nblk of the first term, nblk of the second
constexpr int LL_PARTIALS = 8, LL_MAX_BLOCKS = 256;
constexpr size_t HSMALL_OFF = HSCAL_OFF + HSCAL_BYTES;
// hSmall, the one-launch small path's staging (small.hip): [0, 2) the log-likelihood terms, results of a query, inputs
constexpr int SMALL_KTA = 16;                                   // SMALL_POINTS x GPE_MAX_P
constexpr int SMALL_POINTS = SEQ_WORDS;                         // points of one small-path query
constexpr int SMALL_VAR = SMALL_KTA + SMALL_POINTS * GPE_MAX_P; // SMALL_POINTS
constexpr int SMALL_IN = 256;                                   // obs_mean ((n + 1) x P) or query points (M x D) in
constexpr int SMALL_IN_DOUBLES = 1024;
constexpr int SMALL_DOUBLES = SMALL_IN + SMALL_IN_DOUBLES;
constexpr int SMALL_MAX_N = 256, SMALL_ADD_MAX_P = 3; // the small path's largest order (small.hip: SM_NBLK * NB) and add_sample's P
constexpr size_t PINNED_BYTES = HSMALL_OFF + sizeof(double) * SMALL_DOUBLES;

inline int* info(char* pinned) { return (int*)pinned; }
inline unsigned long long* seq(char* pinned) { return (unsigned long long*)(pinned + SEQ_OFF); }
inline double* hscal(char* pinned) { return (double*)(pinned + HSCAL_OFF); }
inline double* ll_partials(char* pinned) { return hscal(pinned) + LL_PARTIALS; }
inline double* small(char* pinned) { return (double*)(pinned + HSMALL_OFF); }
inline double* small_kta(char* pinned) { return small(pinned) + SMALL_KTA; }
inline double* small_var(char* pinned) { return small(pinned) + SMALL_VAR; }
inline double* small_in(char* pinned) { return small(pinned) + SMALL_IN; }

static_assert(SEQ_WORDS * sizeof(unsigned long long) <= HSCAL_OFF - SEQ_OFF, "the sequence words end in front of hScal");
static_assert(LL_PARTIALS >= 2 && LL_PARTIALS + 2 * LL_MAX_BLOCKS <= HSCAL_DOUBLES, "both runs of partials end inside hScal");
static_assert(SMALL_KTA >= 2 && SMALL_VAR + SMALL_POINTS <= SMALL_IN, "kta and var lie behind the terms and end in front of the inputs");
static_assert((SMALL_MAX_N + 1) * SMALL_ADD_MAX_P <= SMALL_IN_DOUBLES, "add_sample stages (n + 1) x P, n <= SMALL_MAX_N, P <= 3");
static_assert(PINNED_BYTES == 128 + 8192 + 8 * (256 + 1024), "the pinned block: 18,560 bytes");

} // namespace shell
