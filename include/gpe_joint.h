/*
 * gpe_joint.h — the JOINT posterior over a batch of query points: predictive covariance, function draws, arg-max per draw.
 *
 * gpe_query_batch (gpe.h) returns the marginals mu(v_m), sigma^2(v_m) of limbo::model::GP::query (src/limbo/model/gp.hpp:
 * 159-191: _mu :613-616, _sigma :618-624).  The quantity it forms on the way, Z = L^-1 k(X, V) (gp.hpp:620 for every point),
 * is what the joint posterior N(mu, Sigma), Sigma = K(V, V) - Z^T Z, is made of.  The reference has no such call; the entry
 * points below rest on the same lines of gp.hpp and keep their conventions (gpe.h: column-major, host pointers, status).
 *
 * Semantics, for a computed model (N samples, P outputs) and M points V (row-major M x D):
 *   kta[m + M p]  = k(X, v_m)^T alpha_p — bitwise what gpe_query_batch returns for the same batch (the same launches); the mean
 *                   functor is added by the caller (gp.hpp:615).
 *   cov[a + ldc b] = k(v_a, v_b) - (L^-1 k_a).(L^-1 k_b) + jitter [a == b], full symmetric (bitwise cov == cov^T).  k(v, v) is the
 *                   kernel WITHOUT noise (gp.hpp:618-624 calls the functor without indices).  No clamp: cov[m, m] is
 *                   gpe_query_batch's var[m] up to summation order; the clamp of gp.hpp:623 and the + noise of gp.hpp:166 stay
 *                   with the caller.  One Sigma serves all P outputs.
 *   jitter >= 0     is added to the diagonal before Sigma is returned or factorised: `noise` for draws of noisy observations, a
 *                   small value for draws of f.  There is no hidden default.
 *   draws           C = chol(Sigma + jitter I), F[m + M (s + S p)] = mean_q[m + M p] + kta[m + M p] + sum_j C[m, j] Z[j + M (s + S p)].
 *                   The standard normals Z are the CALLER's (no device random numbers): a draw is a deterministic function of
 *                   (model, V, jitter, Z), bitwise reproducible from call to call.  mean_q = m(v) evaluated by the caller (NULL: 0).
 *   argmax[s + S p] = the index of the largest F[:, s, p], the lowest one on exact ties; fmax its value.
 *   status          0; > 0: the 1-based first non-positive pivot of Sigma + jitter I (F, argmax, fmax are then undefined); < 0:
 *                   GPE_ERR_STATE before gpe_compute, GPE_ERR_ARG for M < 0, S < 0, a jitter that is negative or not finite, or M
 *                   above gpe_joint_max_points; GPE_ERR_UNSUPPORTED for GPE_KERNEL_HOST_K handles.  M = 0 is a no-op returning 0.
 *   The model is not changed: gpe_epoch does not move, later queries answer bitwise what they answered before.
 *
 * Limits.  All M rows of Z^T are resident at once, so M <= gpe_joint_max_points = min(2^28 / N rounded down to 64, 16 384):
 * 16 384 points for N <= 16 384.  Sigma's k range is split over workgroups by a plan that depends on M (gpe_debug_cov_plan), so
 * the same point inside another batch is NOT bitwise the same (it agrees to rounding); the same batch is, call after call.
 * The split is the default while Sigma has fewer lower 128 x 128 tiles than two per compute unit (M < ~4000 on 256 CUs); from
 * there on, and always under GPE_JOINT_SPLITK=0, Sigma is formed by the composed path (kernel-matrix build on V, then the
 * triangular matrix-core update with k = N, then the mirror) — the baseline the split was measured against
 * (profiles/joint_posterior_timing.json); GPE_JOINT_SPLITK=1 forces the split.  With fewer samples than one 256-column outer
 * panel the N x M layout of the batched query and the composed path serve the call.
 */
#ifndef GPE_JOINT_H
#define GPE_JOINT_H

#include "gpe.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kta: M x P or NULL; cov: M x M (ldc >= M) or NULL */
int gpe_joint_query(gpe_handle h, const double* Xq_rowmajor, int64_t M, double jitter, double* kta, double* cov, int64_t ldc);
/* mean_q: M x P or NULL; Z: M x S x P (m fastest); F: M x S x P or NULL; argmax, fmax: S x P or NULL.  With F == NULL only the
 * arg-max leaves the device. */
int gpe_joint_draws(gpe_handle h, const double* Xq_rowmajor, int64_t M, double jitter, const double* mean_q, const double* Z, int S,
                    double* F, int64_t* argmax, double* fmax);
/* the cap on M for the handle's current N */
int gpe_joint_max_points(gpe_handle h, int64_t* M_max);
/* Instrumentation: while gpe_set_profiling is on, the phases of the handle's last joint call in ms — { Z = L^-1 k(X, V) with the
 * cross kernel and kta, Sigma, the factorisation (host clock: it runs in the scratch context), the draws with the arg-max }. */
int gpe_joint_phase_ms(gpe_handle h, double* ms4);
/* Test hook, host only: the launch plan of Sigma's product for M points, N samples and `cus` compute units.  One row of 5 int64
 * per workgroup, in launch order: { tile row i, tile column j <= i (128 x 128 tiles of the lower triangle), k0, k1, partial slot }.
 * Every (tile, k) is covered once; k0 is a multiple of 16; a tile's partials are added in ascending slot = ascending k0.
 * Returns the number of rows (out may be null or too small: nothing beyond cap_rows is written), -1 for bad arguments. */
int gpe_debug_cov_plan(int64_t M, int64_t N, int cus, int64_t* out, int64_t cap_rows);

#ifdef __cplusplus
}
#endif
#endif /* GPE_JOINT_H */
