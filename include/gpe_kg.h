/*
 * gpe_kg.h — the knowledge gradient with correlated beliefs over a finite set of alternatives (Frazier, Powell, Dayanik 2009).
 *
 * Every other acquisition of the engine scores a point from the posterior AT that point.  The knowledge gradient values what one
 * noisy observation at a candidate would teach about OTHER points: the expected rise of the best posterior mean over A
 * alternatives.  It needs no incumbent taken from noisy observations (acqui/ei.hpp's f+).  The reference has no such call; the
 * quantities rest on gp.hpp:613-624 as gpe_query_batch and gpe_joint_query do (gpe.h conventions: column-major, host pointers,
 * status).
 *
 * Semantics, for a computed model (N samples), A alternatives Xa (row-major A x D) and M candidates Xc (row-major M x D), fp64:
 *   a_i         mu_a[i] if mu_a is given — then it IS the mean, complete: nothing is added to it (as mu_q of gpe_select_batch);
 *               NULL: a_i = k(X, xa_i)^T alpha_0 (output 0, no mean functor).
 *   c_im        k(xa_i, xc_m) - Zt_a[i, :] . Zt_c[m, :],  Zt[p, :] = L^-1 k(X, p)      (the kernel WITHOUT noise, as gpe_joint.h)
 *   s_m         k(xc_m, xc_m) - |Zt_c[m, :]|^2           gpe_query_batch's var, no clamp
 *   d_m         s_m + obs_noise.  Not above DBL_EPSILON, or not finite: kg[m] = 0 — nothing can be learnt there (gp.hpp:623).
 *   b_i         c_im / sqrt(d_m)
 *   with_self   1: the candidate is one more alternative, line A: (mu_c[m] if given, else k(X, xc_m)^T alpha_0; s_m / sqrt(d_m)).
 *   kg[m]       h(a, b) = E_Z[max_i (a_i + b_i Z)] - max_i a_i >= 0,  Z standard normal.
 *   h           is never formed as that difference (it cancels).  It is the sum over the breakpoints of the upper envelope of the
 *               lines a_i + b_i z:  h = sum (b_next - b_cur) f(-|z|),  f(z) = phi(z) + z Phi(z), every term positive.  The envelope
 *               is a successor chain: for line i, over all j with b_j > b_i, z_ij = (a_i - a_j) / (b_j - b_i); hi_i = min_j z_ij,
 *               succ_i its arg-min.  The chain starts at the smallest slope and follows succ until no steeper line is left; it
 *               adds (b_succ - b_i) f(-|hi_i|) per step.  Adding a constant to every a moves nothing (a enters as differences).
 *   tie rules   succ: the lowest j among equal z_ij.  Start: the smallest slope; among equal slopes the largest a, then the lowest
 *               index (-0.0 and 0.0 are equal).  Lines equal in slope to the current one are never successors.
 *   outputs     kg[M], var_c[M] = s, cov (A x M, column-major, ldc >= A: the unscaled c); each may be NULL.
 *   status      0; GPE_ERR_STATE before gpe_compute (gpe_kg_batch only); GPE_ERR_ARG for A < 1, A > GPE_KG_MAX_ALTERNATIVES,
 *               M < 0, an obs_noise that is negative or not finite, cov with ldc < A, ldb < A; GPE_ERR_UNSUPPORTED for
 *               GPE_KERNEL_HOST_K handles.  M = 0 is a no-op returning 0.
 *   The model is not changed: gpe_epoch does not move, later queries answer bitwise what they answered before.  The same call on
 *   the same inputs is bitwise reproducible, and kg of a candidate is bitwise the same in whatever batch it is asked (the tile of
 *   every product comes from N alone, the k range of the cross-covariance is not split, the envelope is one workgroup's fixed
 *   order; no floating-point atomics).
 *
 * Limits.  A <= 2048: a candidate's lines, breakpoints and successors sit in one workgroup's LDS.  M is unbounded: the candidates
 * stream in chunks as gpe_query_batch's points do; the alternatives' Zt_a (A x N) stays resident for the call.
 *
 * Cost.  One pass of the query family's chunk pipeline for the alternatives; per chunk of candidates the same pass (2 M N^2 flops of
 * panel solve on the matrix cores), the cross-covariance 2 A M N flops there too, and the envelope: A^2 pair steps
 * per candidate — one fp64 division each on the vector units — then a walk of at most A steps by one lane.  The walk is bounded by
 * the line count whatever the inputs (NaN, inf).
 */
#ifndef GPE_KG_H
#define GPE_KG_H

#include "gpe.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPE_KG_MAX_ALTERNATIVES 2048

int gpe_kg_batch(gpe_handle h, const double* Xa_rowmajor, int64_t A, const double* mu_a, const double* Xc_rowmajor, int64_t M,
                 const double* mu_c, double obs_noise, int with_self, double* kg, double* var_c, double* cov, int64_t ldc);
/* The envelope alone on beliefs the caller computed: a[A] the means, B (A x M, column-major, ldb >= A) the slopes, ALREADY scaled
 * (column m is b of candidate m).  kg[m] = h(a, B[:, m]); nseg[m] (may be NULL) = the steps of the chain = the breakpoints of the
 * envelope.  Any handle of the device serves, computed or not.  Serves every Gaussian belief: other kernels, the sparse model. */
int gpe_kg_envelope(gpe_handle h, const double* a, int64_t A, const double* B, int64_t ldb, int64_t M, double* kg, int32_t* nseg);
/* Instrumentation: while gpe_set_profiling is on, the phases of the handle's last gpe_kg_batch in ms — { the alternatives' pass;
 * the candidates' solves with the cross-covariance; the envelopes; the read-back }, summed over the chunks. */
int gpe_kg_phase_ms(gpe_handle h, double* ms4);

#ifdef __cplusplus
}
#endif
#endif /* GPE_KG_H */
