/*
 * gpe_query_grad.h — the posterior over a batch of query points TOGETHER WITH ITS GRADIENT in the point: what a gradient
 * optimiser of an acquisition function consumes (limbo's acqui functors take `gradient`, opt::Rprop / NLOptGrad / Adam ask for it).
 *
 * gpe_query_batch (gpe.h) returns k^T alpha_p and var = k(v, v) - |L^-1 k|^2 for every point v (gp.hpp:613-624).  With
 * k_i = k(v, x_i) and w = L^-T (L^-1 k) = K^-1 k:
 *   d (k^T alpha_p) / dv = sum_i alpha_ip  d k_i / dv
 *   d var / dv           = -2 sum_i w_i    d k_i / dv          (k(v, v) is constant for every kernel with device code)
 * and every kernel with device code has  d k(v, x) / dv = g(z) Mm (v - x),  z = (v - x)^T Mm (v - x):
 *   Mm = diag(ell_d^-2) (SE-ARD), diag(ell_d^-2) + Lambda Lambda^T (SE-ARD with Lambda), l^-2 I (Exp, Matern-5/2, Matern-3/2);
 *   g  = -sf2 e^{-z/2} (SE-ARD, Exp),  -(5/3) sf2 (1 + sqrt(5 z)) e^{-sqrt(5 z)} (Matern-5/2),  -3 sf2 e^{-sqrt(3 z)} (Matern-3/2)
 * — all finite and continuous at z = 0: a query point on a sample is no special case.
 *
 * Semantics, for a computed model (N samples, P outputs, D inputs) and M points V (row-major M x D), conventions of gpe_joint.h:
 *   kta[m + M p]            = k(X, v_m)^T alpha_p;      var[m] = k(v_m, v_m) - |L^-1 k(X, v_m)|^2
 *   dkta[m + M (d + D p)]   = d (k^T alpha_p) / d v_d at v_m;      dvar[m + M d] = d var / d v_d at v_m
 *   No mean functor (nor its derivative), no clamp of the variance, no + noise: those stay with the caller (gp.hpp:615, :623, :166).
 *   Any of the four outputs may be NULL (all four: the call checks its arguments and returns).
 *   The model is not changed: gpe_epoch does not move, the log-likelihood and later queries are bitwise what they were.
 *   status: 0; GPE_ERR_STATE before gpe_compute; GPE_ERR_ARG for M < 0 or a null Xq with M > 0; GPE_ERR_UNSUPPORTED for
 *   GPE_KERNEL_HOST_K handles (no device code for the kernel, hence none for its derivative).  M = 0 returns 0 and does nothing.
 *
 * Bitwise contracts:
 *   - the same call twice gives the same bits (segments of the samples are added in a fixed order, no floating-point atomics);
 *   - a point's four answers do not depend on the batch it is asked in: every tile and every segment count is picked from N alone;
 *   - the call always takes the blocked path of the batched query, never its one-launch paths for a handful of points.  kta and var
 *     are therefore bitwise gpe_query_batch's for M > 8 (the same launches); for M <= 8 they agree to rounding.
 *
 * Path.  Zt = Kst L^-T as in gpe_query_batch; one more triangular solve of the same shape, Wt = Zt L^-1 = (K^-1 k)^T, from the
 * last outer panel to the first; then ONE pass over Wt and alpha that recomputes z from the coordinates (qgrad.hip).  dkta alone
 * needs no solve at all.  Where the transposed layout does not serve the model (fewer samples than one outer panel,
 * GPE_QUERY_T=0, an unusual panel width) and dvar is asked for, K^-1 is formed once by the engine's own inversion and
 * Wt = Kst K^-1 is one product.  STATE SIDE EFFECT of that case only: the handle then holds K^-1 (as after
 * gpe_compute_inv_kernel), cached until K changes; no answer of any call depends on whether it is cached.
 */
#ifndef GPE_QUERY_GRAD_H
#define GPE_QUERY_GRAD_H

#include "gpe.h"

#ifdef __cplusplus
extern "C" {
#endif

int gpe_query_batch_grad(gpe_handle h, const double* Xq_rowmajor, int64_t M,
                         double* kta,   /* M x P or NULL      : kta[m + M p]                                   */
                         double* var,   /* M or NULL                                                           */
                         double* dkta,  /* M x D x P or NULL  : dkta[m + M (d + D p)] = d(k^T alpha_p)/d v_d   */
                         double* dvar); /* M x D or NULL      : dvar[m + M d]                                  */
/* Instrumentation: while gpe_set_profiling is on, the phases of the handle's last gpe_query_batch_grad call in ms, summed over
 * its chunks — { the forward part (cross kernel, kta, Zt, var), the backward solve (or the product with K^-1), the gradient
 * kernel with its fold }. */
int gpe_query_grad_phase_ms(gpe_handle h, double* ms3);

#ifdef __cplusplus
}
#endif
#endif /* GPE_QUERY_GRAD_H */
