/*
 * gpe_cei.h — constrained expected improvement in the log domain.
 *
 * Every other acquisition of the engine scores objectives only.  This one scores "maximise f where c_1 .. c_C hold": the expected
 * improvement of the objective times the probability that every constraint is met, independent Gaussians all.  The reference's side
 * of it is experimental/acqui/eci.hpp (P(feasible) EI, one constraint, threshold 1) under experimental/bayes_opt/cboptimizer.hpp.  Its
 * value s (phi(z) + z Phi(z)) is exactly 0 in double below z = -38.6 and its gradient with it: a flat plateau over most of the box
 * while no feasible point is known.  Here the LOGARITHM is computed, from forms whose terms are all positive, so that value and
 * partials stay finite and accurate however far the candidate lies from the incumbent (gpe.h conventions: column-major, host
 * pointers, status).
 *
 * Semantics.  The objective is MAXIMISED.  s are STANDARD DEVIATIONS.
 *   objective    belief (mu0, s0), incumbent f_best, offset xi:  d = mu0 - f_best - xi,  z = d / s0
 *   constraints  k = 1 .. C <= GPE_CEI_MAX_CONSTRAINTS: belief (mu_k, s_k), threshold t_k; feasible when c_k >= t_k (a "<=" constraint
 *                is the caller's sign flip; the reference's _pf is t = 1):  u_k = (mu_k - t_k) / s_k
 *   h(z)         phi(z) + z Phi(z) = EI / s0.  For z < 0, x = -z, Mills' ratio R(x) = Phi(-x) / phi(x):
 *                  h(z) = Phi(z) T(x),   T(x) = 1 / R(x) - x = 1 / (x + 2 / (x + 3 / (x + ...)))      every partial quotient > 0
 *                so log h = log Phi(z) + log T(x), Phi / h = 1 / T, phi / h = 1 / (R T): finite, growing like |z| and z^2.
 *   logcei       [with_ei] (log s0 + log h(z)) + sum_k log Phi(u_k)
 *   terms        M x (1 + C) column-major, optional: log EI (0 without with_ei), then each log Phi(u_k): which constraint binds
 *   partials     M x (2 + 2 C) column-major, optional: d/d mu0, d/d s0, d/d mu_1 .. mu_C, d/d s_1 .. s_C of logcei:
 *                  d/d mu0 = Phi(z) / (s0 h(z))      d/d s0 = phi(z) / (s0 h(z))
 *                  d/d mu_k = lambda(u_k) / s_k      d/d s_k = -u_k lambda(u_k) / s_k,   lambda = phi / Phi (1 / R(-u) for u < 0)
 *   with_ei = 0  no feasible incumbent yet: the objective's term and its two partials are 0, the value is the log-probability of
 *                feasibility alone; f_best, xi and the objective's belief are not read.
 *   s0 = 0       d > 0: log d, d/d mu0 = 1 / d, d/d s0 = 0;  d <= 0: -inf, both partials 0 (a point without uncertainty and
 *                without improvement: the reference returns 0 there).
 *   s_k = 0      the term is 0 when mu_k >= t_k and -inf otherwise; its partials are 0 in both cases.
 *   NaN          a NaN in any belief of a candidate gives NaN for that candidate alone.
 *   large |z|    finite |z| and |u_k| up to 1e100 give finite values and partials: below the crossover z < -3 nothing like
 *                1 - x R(x) or phi + z Phi is formed.  mu = -inf gives -inf, mu0 = +inf gives +inf, never NaN.
 *   No input makes a loop longer: the continued fraction has a fixed depth chosen from the crossover alone.
 *   The model is not changed: gpe_epoch does not move, later queries answer bitwise what they answered before.  The same call on
 *   the same inputs is bitwise reproducible and a candidate's numbers are bitwise the same in whatever batch it is asked: one thread
 *   scores one candidate in an order fixed by C alone; the tile of every product of the solves comes from N alone (gpe_kg.h); no
 *   atomics.
 *   C = 0 is legal: with_ei = 1 then gives the plain log expected improvement.
 *
 * Cost.  M (1 + C) evaluations, each an exp + erfc + log group or a fixed continued fraction + log, in fp64 on the vector units;
 * gpe_logcei_batch adds gpe_query_batch's solves, 2 M N^2 flops on the matrix cores.
 */
#ifndef GPE_CEI_H
#define GPE_CEI_H

#include "gpe.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPE_CEI_MAX_CONSTRAINTS 16

/* The kernel alone on beliefs the caller computed.  mu0, s0: M each (may be NULL when with_ei = 0); mu_c, s_c: M x C column-major
 * (may be NULL when C = 0); thr: C thresholds.  logcei: M; terms (M x (1 + C)) and partials (M x (2 + 2 C)), column-major, may be
 * NULL.  Any handle of the device serves, computed or not: independently fitted objective and constraint models, the sparse model,
 * any Gaussian belief.  The candidates go 16 384 at a time.  GPE_ERR_ARG: C outside [0, GPE_CEI_MAX_CONSTRAINTS], a threshold that
 * is not finite, an f_best or xi that is not finite while with_ei, a negative s (a NaN s is a belief like any other: NaN out), M < 0,
 * NULL where data is needed.  These checks precede everything that needs the device: with M = 0 the call IS the argument check and
 * does nothing else; h may then be NULL.  GPE_ERR_UNSUPPORTED for GPE_KERNEL_HOST_K handles. */
int gpe_logcei_values(gpe_handle h, int with_ei, double f_best, double xi, int C, const double* thr, const double* mu0, const double* s0,
                      const double* mu_c, const double* s_c, int64_t M, double* logcei, double* terms, double* partials);

/* One computed handle whose output out0 is the objective and whose outputs con_outs[0 .. C) are the constraints: pairwise distinct,
 * inside [0, P).  One factorisation and one solve serve all and they share sigma (limbo's GP with dim_out > 1: what a cboptimizer
 * constraint model is).  The candidates Xc (row-major M x D) stream through gpe_query_batch's chunk pipeline; the kernel runs on
 * each chunk's means and variance where they lie, nothing returns to the host in between.
 *   mean_add   M x (1 + C) column-major or NULL: the mean functor's values of (out0, con_outs...), added to k^T alpha on the device
 *   s^2        (var > DBL_EPSILON ? var : 0) + var_add — the clamp of gp.hpp:621-623; var_add = 0: the latent function, var_add =
 *              the kernel's noise: the observation; every s is sqrt(s^2)
 *   logcei, terms, partials   as above, each may be NULL (d/d s0 and d/d s_k apart: d/d s of the shared sigma is their sum)
 *   mu, var    optional read-backs: mu (M x (1 + C) column-major) = k^T alpha + mean_add of (out0, con_outs...); var (M) =
 *              gpe_query_batch's var — no clamp, nothing added
 * Status: GPE_ERR_STATE before gpe_compute; GPE_ERR_UNSUPPORTED for GPE_KERNEL_HOST_K handles; GPE_ERR_ARG for outputs that repeat
 * or lie outside [0, P), C outside [0, GPE_CEI_MAX_CONSTRAINTS], a threshold, or with with_ei an f_best or xi, that is not finite,
 * M < 0, a var_add that is negative or not finite.  M = 0 is a no-op. */
int gpe_logcei_batch(gpe_handle h, int with_ei, int out0, double f_best, double xi, int C, const int* con_outs, const double* thr,
                     const double* Xc_rowmajor, int64_t M, const double* mean_add, double var_add, double* logcei, double* terms,
                     double* partials, double* mu, double* var);

/* Instrumentation: while gpe_set_profiling is on, the phases of the handle's last gpe_logcei_batch in ms — { the solves (head, solve,
 * variance); the kernel; the read-back }, summed over the chunks. */
int gpe_cei_phase_ms(gpe_handle h, double* ms3);

#ifdef __cplusplus
}
#endif
#endif /* GPE_CEI_H */
