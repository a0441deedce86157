/*
 * gpe_batch_select.h — greedy batch selection with hallucinated observations: q proposals from M candidates and ONE model state.
 *
 * The batch loop is "propose q points -> evaluate them in parallel -> gpe_add_samples (gpe_append.h)".  gpe_joint_draws and the
 * path sets (gpe_pathwise.h) propose at random; this call proposes deterministically: pick the acquisition maximiser, condition
 * the posterior VARIANCE on an observation there (the mean does not move: nothing has been observed), pick again.  With the
 * UCB rule this is GP-BUCB, with EI the kriging believer, with the variance rule a pivoted Cholesky / max-variance design.  The
 * reference has no such call; the quantities rest on gp.hpp:613-624 as gpe_query_batch and gpe_joint_query do (gpe.h conventions:
 * column-major, host pointers, status).
 *
 * Semantics, for a computed model (N samples, P outputs) and M candidates V (row-major M x D), fp64 throughout:
 *   rule        GPE_SELECT_UCB  score = mu + beta sqrt(s2)                                  beta_or_offset = beta >= 0
 *               GPE_SELECT_EI   sigma = sqrt(s2); 0 where sigma < 1e-10, else X Phi(X / sigma) + sigma phi(X / sigma),
 *                               X = mu - offset (acqui/ei.hpp: _value)                       beta_or_offset = f+ + jitter
 *               GPE_SELECT_VAR  score = s2
 *   mu_q        M doubles or NULL.  NULL: mu[m] = k(X, v_m)^T alpha_0 (output 0, no mean functor).  Otherwise it IS mu, complete:
 *               the caller has added the mean functor and applied its aggregator; nothing is added to it.
 *   var_add     >= 0: s2[m] = (var_t[m] <= DBL_EPSILON ? 0 : var_t[m]) + var_add — the clamp of gp.hpp:623 and the + noise of
 *               gp.hpp:166.  It enters the score only, never the recursion.
 *   obs_noise   >= 0: the noise lambda of the hallucinated observation.
 *   distinct    1: a picked candidate is left out of later rounds.  0: with lambda > 0 a candidate may be picked again (a replicate).
 *   recursion   var_0[m] = k(v_m, v_m) - |Zt[m, :]|^2, Zt[m, i] = (L^-1 k(X, v_m))_i, no clamp (gpe_query_batch's var up to
 *               summation order).  For t = 0 .. q-1:
 *                 j_t      = argmax_m score(mu[m], s2_t[m])      the lowest index on exact ties
 *                 c[m]     = k(v_m, v_j) - Zt[m, :].Zt[j, :] - sum_{s<t} W[m, s] W[j, s]      (the kernel WITHOUT noise)
 *                 piv      = c[j_t] + obs_noise                  not positive or not finite: stop, status = t + 1
 *                 W[m, t]  = c[m] / sqrt(piv),   var_{t+1}[m] = var_t[m] - W[m, t]^2
 *   outputs     idx[q], score[q] (the winning score of each round), var_out[M] = var_q (no clamp), W (M x q, column-major, ldw >= M);
 *               each may be NULL.
 *   status      0; t + 1 > 0: the first round whose pivot is not positive (rounds < t are valid; idx and score of round t are set,
 *               column t of W is not); GPE_ERR_STATE before gpe_compute; GPE_ERR_ARG for M < 0, q < 0, q > 1024, distinct with
 *               q > M, a beta, var_add or obs_noise that is negative or not finite (EI's offset may be negative; a value that is
 *               not finite is refused under every rule), an unknown rule, W with ldw < M, or M above gpe_joint_max_points (all rows
 *               of Zt are resident at once); GPE_ERR_UNSUPPORTED for GPE_KERNEL_HOST_K handles.  M = 0 or q = 0 is a no-op
 *               returning 0.
 *   The model is not changed: gpe_epoch does not move, later queries answer bitwise what they answered before.  The same call on
 *   the same inputs is bitwise reproducible (fixed-order reductions, no floating-point atomics).
 *
 * Cost.  One pass of the query family's chunk pipeline (Zt, kta, var_0), then per round ONE covariance column, a matrix-vector
 * product over Zt: M N 8 bytes of reads, its k range split over workgroups by a plan (gpe_debug_select_plan) and folded in
 * ascending slot.  The q rounds are enqueued at once; the pick of a round is read from device memory by the next launch.
 */
#ifndef GPE_BATCH_SELECT_H
#define GPE_BATCH_SELECT_H

#include "gpe.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPE_SELECT_UCB 0
#define GPE_SELECT_EI 1
#define GPE_SELECT_VAR 2
#define GPE_SELECT_MAX_ROUNDS 1024

int gpe_select_batch(gpe_handle h, const double* Xq_rowmajor, int64_t M, int q, int rule, double beta_or_offset, const double* mu_q,
                     double var_add, double obs_noise, int distinct, int64_t* idx, double* score, double* var_out, double* W, int64_t ldw);
/* Instrumentation: while gpe_set_profiling is on, the phases of the handle's last gpe_select_batch in ms — { Zt with the cross
 * kernel, kta and var_0; the q rounds; the read-back }. */
int gpe_select_phase_ms(gpe_handle h, double* ms3);
/* Test hook, host only: the launch plan of one round's column product for M candidates, N samples and `cus` compute units.  One
 * row of 5 int64 per workgroup, in launch order: { m0, m1, k0, k1, partial slot } — the workgroup leaves sum_{k0 <= i < k1}
 * Zt[m, i] z[i] for m0 <= m < m1 in partial vector `slot`.  Every (m, k) is covered once; k0 is a multiple of 16; the partials
 * of an m are added in ascending slot = ascending k0.  Returns the number of rows (out may be null or too small: nothing beyond
 * cap_rows is written), -1 for bad arguments. */
int gpe_debug_select_plan(int64_t M, int64_t N, int cus, int64_t* out, int64_t cap_rows);

#ifdef __cplusplus
}
#endif
#endif /* GPE_BATCH_SELECT_H */
