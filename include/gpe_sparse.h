/*
 * gpe_sparse.h — the sparse pseudo-input GP (SPGP / "FITC", Snelson & Ghahramani 2005) posterior on the device.
 *
 * The counterpart of limbo's experimental model src/limbo/experimental/model/spgp.hpp: N training points are summarised by
 * M << N pseudo-inputs Xb, every factorisation is M x M, the cost is O(N M^2) time and O(N + M^2) memory instead of the exact
 * model's O(N^3) and O(N^2) (gpe.h).  The conventions of gpe.h hold (column-major, host pointers, int status); every entry
 * names the lines of spgp.hpp it replaces.
 *
 * Kernel.  SE-ARD in the SPGP parametrisation of spgp.hpp:612-634:  k(a, b) = c exp(-1/2 sum_d b_d (a_d - b_d)^2), that is
 * GPE_KERNEL_SE_ARD with l_d = b_d^(-1/2) and sigma_f^2 = c.  log_b[D], log_c and log_sig are in log-space as the reference's
 * HyperParams (spgp.hpp:94-101); sig = exp(log_sig) is the noise VARIANCE (the reference's comments at :334-335 have c and
 * sig exchanged); jitter is the reference's _del (Params::model_spgp::jitter(), :394, :467).
 *
 * What gpe_sp_compute leaves (spgp.hpp:394-406), for X (N x D), Xb (M x D) and obs_zm (N x P):
 *   L    = chol(K(Xb, Xb) + jitter I)                     M x M lower            (:394-395)
 *   V    = L^-1 K(Xb, X)                                   M x N, never resident for more than one chunk of columns (:396-398)
 *   ep_n = 1 + (c - sum_i V[i, n]^2) / sig                 N                      (:399)
 *   A    = sig I + sum_n V[:, n] V[:, n]^T / ep_n,  Lm = chol(A)                  (:402, :405)
 *   bet  = Lm^-1 sum_n V[:, n] y_n / ep_n                  M x P                  (:403, :406)
 *
 * Semantics.
 *   Mean and noise.  gpe_sp_predict returns mu[t + T p] = bet_p^T Lm^-1 L^-1 k(Xb, x_t) WITHOUT the mean functor (:603 stays
 *     with the caller) and s2[t] = c - |lst|^2 + sig |lmst|^2 with lst = L^-1 k(Xb, x_t), lmst = Lm^-1 lst (:597-599, :608)
 *     WITHOUT the "+ sig" the reference adds once a model has been optimised (:608, _optimized) and without a clamp: the caller
 *     adds both.
 *   Likelihood.  gpe_sp_nlml returns, per output p, the NEGATIVE log marginal likelihood fw of spgp.hpp:491,
 *       sum log diag(Lm) + (n - m)/2 log sig + (yh_p.yh_p - bet_p.bet_p) / (2 sig) + 1/2 sum log ep + n/2 log 2 pi,
 *     yh = y / sqrt(ep), with the REAL (n - m)/2: the reference writes (n - _m) / 2 on integers and drops a half for odd n - m,
 *     an artefact of the C++ expression, not of the model.  One value per output (the reference's expression only
 *     type-checks for P = 1; with P = 1 it is that value).
 *   Status.  0; > 0: the 1-based first non-positive pivot — of K(Xb, Xb) + jitter I as it is, of A offset by M (M + j); the
 *     model is then not computed.  GPE_ERR_STATE: compute / objective before data, pseudo-inputs and hyper-parameters have all
 *     been set (set_pseudo before set_data as well: it takes D from the data), nlml / predict / get_* before a compute that
 *     returned 0.  GPE_ERR_ARG: null pointers, N < 1, D outside 1 .. 62, P < 1, M < 1, M > N, M > 16 384, values that are not
 *     finite, a jitter below 1e-8 — the dense engine adds noise + 1e-8 to its diagonal (kernel/kernel.hpp:83), so the inner model
 *     over the pseudo-inputs is given noise = jitter - 1e-8 — and ld < M.
 *   Limits.  M <= 16 384.  N is limited by X, obs_zm and ep in device memory (N (D + P + 1) doubles); V exists one chunk of
 *     columns at a time (GPE_SPARSE_CHUNK columns; by default as many as keep the chunk's two M x chunk buffers under 512 MiB,
 *     at most 65 536, a multiple of 64).
 *   Reproducibility.  Every output is bitwise reproducible from call to call, and a handle whose hyper-parameters are rewritten
 *     answers bitwise what a fresh handle with those values answers: the order of every sum over n — over the chunks, over the
 *     slices of a chunk (gpe_debug_gram_plan) and inside a slice — is fixed by the plan; there are no floating-point atomics.
 *     Another chunk length is another summation order: results then agree to rounding, not bitwise.
 *   Independence of the batch.  A prediction does not depend on the batch it is asked in (bitwise): as in the batched query
 *     (csrc/query.hpp, qt_layout) the tile of every product is picked from M alone, never from T.
 *   The hyper-parameter setters do not compute; gpe_sp_set_data / gpe_sp_set_pseudo / gpe_sp_set_hparams invalidate the model.
 *
 * How.  The pseudo-inputs are the samples of a private dense model (gpe.h) that factorises K(Xb, Xb) by the engine's own
 * schedule; a chunk of training rows is a batch of "query points" of that model, so V^T is the Zt of the batched query
 * (csrc/query.hpp) — or, below one 256-column outer panel of pseudo-inputs, V in the N x M layout of its blocked solve.  Per
 * chunk: ep and w = 1 / ep (k_sp_ep), r += V (w y) (k_sp_r), and the weighted Gram A += V diag(w) V^T by the split-k matrix-core
 * kernel k_sp_gram (csrc/sparse.hip) while A has fewer lower 64 x 64 tiles than two per compute unit (M <= 1984 on 256 CUs); from
 * there on, and always under GPE_SPARSE_GRAM=0, by the engine's general product on a weighted copy of V — the baseline the kernel
 * was measured against (profiles/sparse_gp_timing.json); GPE_SPARSE_GRAM=1 forces the kernel.  A is
 * factorised in a second private context whose right-hand sides are r: its forward substitution leaves bet.
 */
#ifndef GPE_SPARSE_H
#define GPE_SPARSE_H

#include "gpe.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpe_sp_ctx* gpe_sp_handle;

int gpe_sp_create(int device_id, gpe_sp_handle* out);
int gpe_sp_destroy(gpe_sp_handle h);
const char* gpe_sp_last_error(gpe_sp_handle h);

/* spgp.hpp:353-366 _init: X N x D row-major, obs_zm = Y - m(X) N x P column-major (:372-379, evaluated by the caller) */
int gpe_sp_set_data(gpe_sp_handle h, const double* X_rowmajor, int64_t N, int D, const double* obs_zm, int P);
/* spgp.hpp:437 _pseudo_samples: M x D row-major (D of the data) */
int gpe_sp_set_pseudo(gpe_sp_handle h, const double* Xb_rowmajor, int64_t M);
/* spgp.hpp:438-440 _b, _c, _sig from their logarithms (:94-101) and _del (:366) */
int gpe_sp_set_hparams(gpe_sp_handle h, const double* log_b, double log_c, double log_sig, double jitter);
/* spgp.hpp:394-406: L, V (chunk by chunk), ep, Lm, bet */
int gpe_sp_compute(gpe_sp_handle h);
/* spgp.hpp:491 fw, per output: out[P] */
int gpe_sp_nlml(gpe_sp_handle h, double* out);
/* spgp.hpp:446-498 _likelihood without the gradient, pseudo-inputs fixed: set_hparams + compute + nlml in one call */
int gpe_sp_objective(gpe_sp_handle h, const double* log_b, double log_c, double log_sig, double jitter, double* nlml);
/* spgp.hpp:597-608 _predict for T points (row-major T x D): mu T x P column-major or NULL, s2 T or NULL */
int gpe_sp_predict(gpe_sp_handle h, const double* Xt_rowmajor, int64_t T, double* mu, double* s2);

/* accessors: _matrixL (:395) and _Lm (:405), lower with the upper part zeroed, ld >= M; _bet (:406) M x P; ep (:399) N */
int gpe_sp_get_L(gpe_sp_handle h, double* L, int64_t ld);
int gpe_sp_get_Lm(gpe_sp_handle h, double* Lm, int64_t ld);
int gpe_sp_get_bet(gpe_sp_handle h, double* bet);
int gpe_sp_get_ep(gpe_sp_handle h, double* ep);

/* Instrumentation: gpe_sp_set_profiling(1) brackets the phases of gpe_sp_compute / gpe_sp_predict with events; ms5 = { K_mn and
 * V (the cross kernel and the solve, all chunks), ep and r, the Gram, the factorisation of A with bet (host clock: it runs in
 * the scratch context), the last gpe_sp_predict } in ms. */
int gpe_sp_set_profiling(gpe_sp_handle h, int on);
int gpe_sp_phase_ms(gpe_sp_handle h, double* ms5);

/* Test hook, host only: the launch plan of the Gram A = sum_n w_n V[:, n] V[:, n]^T for M pseudo-inputs, N points streamed in
 * chunks of `chunk` columns (<= 0: the default for M; rounded up to 64) on `cus` compute units.  One row of 5 int64 per
 * workgroup, in launch order (chunk by chunk, slice by slice): { tile row i, tile column j <= i (64 x 64 tiles of the lower
 * triangle), k0, k1 (the columns [k0, k1) of V, indices into 0 .. N), slot }.  Every (tile, k) is covered once; k0 is a multiple
 * of 64 (16 steps of the 16 x 16 x 4 matrix-core instruction); a tile's partial products are added in ascending slot, which is
 * ascending k0.  A chunk's k range is cut into about 2 cus / (number of lower tiles) slices, none shorter than 256 columns, 64
 * at most.  Returns the number of rows (out may be null or too small: nothing beyond cap_rows is written), -1 for bad arguments. */
int gpe_debug_gram_plan(int64_t M, int64_t N, int64_t chunk, int cus, int64_t* out, int64_t cap_rows);

#ifdef __cplusplus
}
#endif
#endif /* GPE_SPARSE_H */
