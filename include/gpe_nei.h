/*
 * gpe_nei.h — noisy expected improvement in the log domain.
 *
 * Expected improvement takes its incumbent f+ from the caller, in practice the largest NOISY observation — which is biased
 * upwards, so that candidates are compared against a value the function may never have reached.  Noisy expected improvement
 * (Letham, Karrer, Ottoni, Bakshy 2019) averages EI over joint posterior draws of the function at baseline points (the points
 * observed so far, or a pruned subset): every draw carries its own incumbent, and the belief at the candidate is conditioned on that
 * draw.  Conditioning removes most of the variance near the baseline, z = (mean - incumbent) / sd runs to the hundreds below zero
 * and EI as written is exactly 0 there, so the value is computed as a LOGARITHM from gpe_cei.h's forms, whose terms are all
 * positive (gpe.h conventions: column-major, host pointers, status).
 *
 * Semantics.  The objective is MAXIMISED.  A computed model with N samples X and P outputs; `out` is the output scored.
 *   baseline     Xb, row-major B x D, 1 <= B <= GPE_NEI_MAX_BASELINE
 *   normals      Z, B x S column-major, 1 <= S <= GPE_NEI_MAX_SAMPLES: standard normals of the CALLER's (as gpe_joint_draws: there
 *                are no device random numbers); finite
 *   mu_b         k(X, xb_i)^T alpha_out + mean_b[i]                                   (mean_b NULL: 0)
 *   Sigma_b      k(Xb, Xb) - Zt_b Zt_b^T + jitter I = L_b L_b^T, Zt_b = (L^-1 k(X, Xb))^T   (the kernel WITHOUT noise, as gpe_joint.h;
 *                jitter >= 0, no hidden default)
 *   F[:, s]      mu_b + L_b Z[:, s];   fplus[s] = max_i F[i, s]
 *   per candidate x:
 *   mu           k(X, x)^T alpha_out + mean_add;   var = gpe_query_batch's var (no clamp)
 *   c            k(Xb, x) - Zt_b Zt_x^T  (B);   u = L_b^-1 c
 *   cmean[s]     mu + u . Z[:, s]: the mean at x given draw s, the baseline values observed with variance `jitter`
 *   cvar         var - |u|^2: the variance at x given ANY draw — formed as this difference of a variance and a sum of squares,
 *                never through Sigma_b^-1;   sd = sqrt(cvar > DBL_EPSILON ? cvar : 0)   (the clamp of gp.hpp:623)
 *   term_s       log sd + log h((cmean[s] - fplus[s] - xi) / sd),  h(z) = phi(z) + z Phi(z): below z = -3 from Mills' ratio as a
 *                continued fraction of fixed depth whose partial quotients are all positive, above from the direct forms (gpe_cei.h)
 *   lognei       log((1 / S) sum_s exp(term_s)): the maximum first, then the sum in an order fixed by S alone.  The plain value is
 *                exp(lognei), taken by the caller.
 *   (cmean, cvar) are exactly the posterior at x of the model that also holds the fantasies (Xb, F[:, s]) observed with noise
 *   variance `jitter`.
 *   sd = 0       term_s = log(cmean[s] - fplus[s] - xi) if that is > 0, else -inf   (gpe_cei.h's s0 = 0 rule)
 *   all -inf     lognei = -inf.
 *   NaN          a NaN in a candidate's belief (a mean, sd) gives NaN for that candidate alone (value and terms).
 *   mean = +inf  lognei = +inf, never NaN.
 *   large |z|    finite |z| up to 1e100 give finite values.
 *   No input makes a loop longer.
 *   The model is not changed: gpe_epoch does not move, later gpe_query_batch, gpe_joint_query and gpe_joint_draws answer bitwise what
 *   they answered before.  The same call on the same inputs is bitwise reproducible, and a candidate's lognei, cvar and cmean are
 *   bitwise the same asked alone, in halves or in one batch: the tile of every product comes from N or B alone, no k range is
 *   split, one wave scores one candidate; no floating-point atomics.
 *
 * Cost.  Once per call the baseline: 2 B N^2 flops of solves, B^2 N for Sigma_b, B^3 / 3 for its factor, B^2 S for the draws.  Per
 * candidate gpe_query_batch's 2 N^2, then 2 B N (the cross-covariance), B^2 (the solve by L_b), 2 B S (the means) on the matrix
 * cores and S evaluations of log h on the vector units.
 */
#ifndef GPE_NEI_H
#define GPE_NEI_H

#include "gpe.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPE_NEI_MAX_BASELINE 1024
#define GPE_NEI_MAX_SAMPLES 1024

/* The kernel alone on conditional beliefs the caller computed: fplus[S]; cmean S x M column-major, ldm >= S (what lies behind row S
 * of a column is not read); csd[M] >= 0, STANDARD DEVIATIONS.  lognei[M]; terms (S x M, ld = S) may be NULL.  Any handle of the device
 * serves, computed or not.  The candidates go 16 384 at a time.  GPE_ERR_ARG: S outside [1, GPE_NEI_MAX_SAMPLES], an fplus or xi that
 * is not finite, a negative csd (a NaN csd is a belief like any other: NaN out), ldm < S, M < 0, NULL where data is needed.  These
 * checks precede everything that needs the device: with M = 0 the call IS the argument check and does nothing else; h may then be
 * NULL.  GPE_ERR_UNSUPPORTED for GPE_KERNEL_HOST_K handles. */
int gpe_lognei_values(gpe_handle h, int S, const double* fplus, double xi, const double* cmean, int64_t ldm, const double* csd, int64_t M,
                      double* lognei, double* terms);

/* Fused with the query pipeline.  The baseline is solved, its covariance formed and factored and the draws taken once; the
 * candidates Xc (row-major M x D) then stream through gpe_query_batch's chunk pipeline, and cross-covariance, conditioning and the
 * kernel run on each chunk where it lies.
 *   mean_b     B or NULL, mean_add M or NULL: the mean functor's values of `out` at the baseline and at the candidates
 *   outputs    each may be NULL: lognei[M]; fplus[S]; mu[M] = k^T alpha_out + mean_add; var[M] = gpe_query_batch's var; cvar[M] (no
 *              clamp); cmean (S x M column-major, ldm >= S)
 * Status: 0; > 0: the 1-based first non-positive pivot of Sigma_b + jitter I, as gpe_joint_draws' — no output is written;
 * GPE_ERR_STATE before gpe_compute; GPE_ERR_UNSUPPORTED for GPE_KERNEL_HOST_K handles; GPE_ERR_ARG for B or S outside their ranges,
 * B above gpe_joint_max_points (the baseline is resident like a joint call's points; below 1024 only for N > 262 144),
 * `out` outside [0, P), a jitter that is negative or not finite, an xi or Z that is not finite, cmean with ldm < S, M < 0, NULL where
 * data is needed.  On an error no output is written.  M = 0 is a no-op. */
int gpe_lognei_batch(gpe_handle h, int out, const double* Xb_rowmajor, int64_t B, const double* mean_b, double jitter, const double* Z, int S,
                     double xi, const double* Xc_rowmajor, int64_t M, const double* mean_add, double* lognei, double* fplus, double* mu,
                     double* var, double* cvar, double* cmean, int64_t ldm);

/* Instrumentation: while gpe_set_profiling is on, the phases of the handle's last gpe_lognei_batch in ms — { the baseline's pass and
 * Sigma_b; its factorisation (host clock) and the draws with their maxima; the candidates' solves with the cross-covariance; the
 * conditioning (the solve by L_b, variance, means); the kernel and the read-back }, the last three summed over the chunks. */
int gpe_nei_phase_ms(gpe_handle h, double* ms5);

#ifdef __cplusplus
}
#endif
#endif /* GPE_NEI_H */
