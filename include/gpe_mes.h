/*
 * gpe_mes.h — max-value entropy search in the log domain.
 *
 * The engine's information-theoretic acquisition: the expected drop in the entropy of the MAXIMUM VALUE y* after an observation at
 * x (Wang & Jegelka 2017), from K samples of y* (gpe_pathwise.h: gpe_paths_argmax's fmax) and the belief (mu, s) at x.  Summed over
 * outputs it is MESMO with per-objective maxima (Belakaria et al. 2019): an acquisition for any number of objectives.  No incumbent
 * enters.  The per-sample term as written, g phi(g) / (2 Phi(g)) - log Phi(g), is 0 / 0 below g = -38.5 and exactly 0 — flat, its
 * gradient with it — above g = +38.6 in double.  Here its LOGARITHM is computed from forms whose terms are all positive on both
 * tails, so that value and partials stay finite and accurate however far the belief lies from the sampled maxima (gpe.h
 * conventions: column-major, host pointers, status).
 *
 * Semantics.  The objective is MAXIMISED.  s are STANDARD DEVIATIONS.
 *   outputs      j = 0 .. J-1, 1 <= J <= GPE_MES_MAX_OUTPUTS: belief (mu_j, s_j)
 *   samples      k = 0 .. K-1, 1 <= K <= GPE_MES_MAX_SAMPLES: ystar[k + K j], the k-th sampled maximum of output j;
 *                g_jk = (ystar_jk - mu_j) / s_j
 *   t(g)         g phi(g) / (2 Phi(g)) - log Phi(g) > 0, falling;  r = t' / t <= 0.  With x = |g|, Mills' ratio R(x) = Phi(-x) / phi(x),
 *                1 / T = x + c2, c2 = 2 / (x + 3 / (x + ...)) (every partial quotient > 0), lambda = phi / Phi:
 *                  g < -3   lambda = x + T,  t = log sqrt(2 pi) + log(x + T) - x T / 2,  t' = -(lambda / 2) c2 T   (-> log x, -1 / x)
 *                  g > +3   Q = phi R,  log t = -g^2 / 2 - log sqrt(2 pi) + log B,  B = g / (2 (1 - Q)) + R (-log1p(-Q) / Q),
 *                           t' / t = -[1 + g (g + phi / (1 - Q))] / (2 (1 - Q) B)                                  (-> -g)
 *                  else     t = g lambda / 2 - log Phi,  t' = -(lambda / 2) (1 + g (g + lambda))
 *   terms        M x J column-major, optional: terms[m, j] = log((1 / K) sum_k t(g_jk)), the log of output j's MES
 *   logmes       log sum_j exp(terms[m, j]).  J = 1: MES.  J > 1: MESMO.  The plain value is exp(logmes), taken by the caller.
 *   partials     M x 2 J column-major, optional: d logmes / d mu_0 .. mu_{J-1}, then d logmes / d s_0 .. s_{J-1}.  With
 *                w_jk = t_jk / sum_k t_jk and W_j = exp(terms_j - logmes):
 *                  d/d mu_j = -(W_j / s_j) sum_k w_jk r_jk  >= 0        d/d s_j = -(W_j / s_j) sum_k w_jk g_jk r_jk
 *   Every sum over k and over j is a log-sum-exp with the maximum taken first, in an order fixed by (J, K) alone.
 *   s_j = 0      output j teaches nothing: its term is -inf and its partials are 0, whatever the order of mu_j and ystar.
 *   all -inf     logmes = -inf, the partials are 0.
 *   NaN          a NaN in any belief of a candidate gives NaN for that candidate alone (value, terms, partials).
 *   mu infinite  mu_j = -inf: term j is -inf; mu_j = +inf: term j and logmes are +inf; never NaN; the partials are 0.
 *   large |g|    finite |g| up to 1e100 give finite values and partials.
 *   No input makes a loop longer: the continued fraction has a fixed depth chosen from the crossover alone.
 *   The model is not changed: gpe_epoch does not move, later queries answer bitwise what they answered before.  The same call on
 *   the same inputs is bitwise reproducible and a candidate's numbers are bitwise the same in whatever batch it is asked: one wave
 *   scores one candidate in an order fixed by (J, K) alone; the tile of every product of the solves comes from N alone (gpe_kg.h);
 *   no atomics.
 *
 * Cost.  M J K evaluations, each a fixed continued fraction of 58 divisions + exp + 2 log, or an exp + erfc + 2 log group, in fp64
 * on the vector units; gpe_mes_batch adds gpe_query_batch's solves, 2 M N^2 flops on the matrix cores.
 */
#ifndef GPE_MES_H
#define GPE_MES_H

#include "gpe.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPE_MES_MAX_OUTPUTS 8
#define GPE_MES_MAX_SAMPLES 1024

/* The kernel alone on beliefs the caller computed.  ystar: K x J column-major; mu, s: M x J column-major.  logmes: M; terms (M x J)
 * and partials (M x 2 J), column-major, may be NULL.  Any handle of the device serves, computed or not: separately fitted models,
 * the sparse model, any Gaussian belief.  The candidates go 16 384 at a time.  GPE_ERR_ARG: J outside [1, GPE_MES_MAX_OUTPUTS], K
 * outside [1, GPE_MES_MAX_SAMPLES], a ystar that is not finite, a negative s (a NaN s is a belief like any other: NaN out), M < 0,
 * NULL where data is needed.  These checks precede everything that needs the device: with M = 0 the call IS the argument check and
 * does nothing else; h may then be NULL.  GPE_ERR_UNSUPPORTED for GPE_KERNEL_HOST_K handles. */
int gpe_mes_values(gpe_handle h, int J, int K, const double* ystar, const double* mu, const double* s, int64_t M, double* logmes,
                   double* terms, double* partials);

/* One computed handle whose outputs outs[0 .. J) are scored: pairwise distinct, inside [0, P).  One factorisation and one solve
 * serve all and they share sigma (limbo's GP with dim_out > 1).  The candidates Xc (row-major M x D) stream through
 * gpe_query_batch's chunk pipeline; the kernel runs on each chunk's means and variance where they lie, nothing returns to the host
 * in between.
 *   mean_add   M x J column-major or NULL: the mean functor's values of outs, added to k^T alpha on the device
 *   s^2        (var > DBL_EPSILON ? var : 0) + var_add — the clamp of gp.hpp:621-623; var_add = 0: the latent function, var_add =
 *              the kernel's noise: the observation; every s_j is sqrt(s^2)
 *   logmes, terms, partials   as above, each may be NULL (the d/d s_j apart: d/d s of the shared sigma is their sum)
 *   mu, var    optional read-backs: mu (M x J column-major) = k^T alpha + mean_add of outs; var (M) = gpe_query_batch's var — no
 *              clamp, nothing added
 * Status: GPE_ERR_STATE before gpe_compute; GPE_ERR_UNSUPPORTED for GPE_KERNEL_HOST_K handles; GPE_ERR_ARG for outputs that repeat
 * or lie outside [0, P), J or K outside their ranges, a ystar that is not finite, M < 0, a var_add that is negative or not finite.
 * On an error no output is written.  M = 0 is a no-op. */
int gpe_mes_batch(gpe_handle h, int J, const int* outs, int K, const double* ystar, const double* Xc_rowmajor, int64_t M,
                  const double* mean_add, double var_add, double* logmes, double* terms, double* partials, double* mu, double* var);

/* Instrumentation: while gpe_set_profiling is on, the phases of the handle's last gpe_mes_batch in ms — { the solves (head, solve,
 * variance); the kernel; the read-back }, summed over the chunks. */
int gpe_mes_phase_ms(gpe_handle h, double* ms3);

#ifdef __cplusplus
}
#endif
#endif /* GPE_MES_H */
