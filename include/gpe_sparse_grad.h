/*
 * gpe_sparse_grad.h — the analytic gradient of the sparse pseudo-input GP's likelihood on the device.
 *
 * The counterpart of the gradient half of `_likelihood_wp` (src/limbo/experimental/model/spgp.hpp:500-580): the derivatives of
 *     F = sum_p nlml_p        (gpe_sp_nlml, gpe_sparse.h, summed over the P outputs)
 * with respect to all (M + 1) D + 2 parameters of the model — the M pseudo-inputs' RAW coordinates, log b_d, log c, log sig
 * (spgp.hpp:94-101) — from one pass over the N training points in chunks, O(N M^2) time and O(M^2 + chunk M) memory: no M x N
 * matrix is ever resident.  The conventions of gpe_sparse.h hold (host pointers, int status, the model's reproducibility).
 *
 * The form (V~ = V / sqrt(ep) and K~ = K(Xb, X) / sqrt(ep) by column, y~ = y / sqrt(ep), Q = K(Xb, Xb) + jitter I, x^ = x sqrt(b)):
 *   M x M, no pass over N:  Li = L^-1, Lmi = Lm^-1, Lti = Lmi Li = (L Lm)^-1 (the reference's invLt, :505) by triangular solves
 *     of the identity;  invQ = Li^T Li,  invA = Lti^T Lti,  b1 = Lti^T bet.
 *   per chunk:  V as gpe_sp_compute forms it (the same cross kernel and solve: ep, Lm and bet came from that V, and the gradient's
 *     large terms cancel only against a V consistent with them),  ILV = Lmi V~ (:483),  B1 = Lti^T ILV (:502),  IQ = Li^T V~ (:504)
 *     on the matrix cores;  per point mu_np = bet_p . ILV_n (:509),  q_n = |ILV_n|^2,  s_n = |IQ_n|^2,
 *     bigsum_n = sum_p (y~ mu / sig - (y~^2 + mu^2) / (2 sig)) + P (1/2 - q_n / 2)      (:515-517),
 *     epc_n = (c / ep_n - sumVsq_n - jitter s_n) / sig                                     (:554-556);
 *     G_jn = K~_jn (P B1_jn - (2 / sig) IQ_jn bigsum_n - sum_p b1_jp (y~_np - mu_np) / sig), never stored, and its row sums
 *     against [1, x^, x^2] (2 D + 1 per pseudo-input: every term of :526-544 that runs over n);
 *     TT += IQ diag(bigsum) IQ^T (:518), the weighted Gram of the model with signed weights.
 *   finish:  the M x M sums against dnnQ (:524, :530-533), the four rescalings (:546-552), dfc (:557-560), dfsig (:562).
 *
 * Reproducibility.  As the model's: every sum over n runs in an order fixed by the chunk length and the slice plans, there are
 * no floating-point atomics; the same call twice is bitwise equal; another GPE_SPARSE_CHUNK agrees to rounding.  Four
 * chunk x M buffers are live (K~, B1, IQ, ILV) beside the model's two, so the gradient's default chunk is as many columns as
 * keep those four under 512 MiB (at most 65 536, a multiple of 64); GPE_SPARSE_CHUNK overrides it as it does the model's.
 */
#ifndef GPE_SPARSE_GRAD_H
#define GPE_SPARSE_GRAD_H

#include "gpe_sparse.h"

#ifdef __cplusplus
extern "C" {
#endif

/* spgp.hpp:500-580: the gradient of sum_p nlml_p of the model as computed.  d_xb: M x D row-major (as gpe_sp_set_pseudo takes
 * the pseudo-inputs), or NULL; d_hp: D + 2 = { d/d log b_0 .. d/d log b_{D-1}, d/d log c, d/d log sig }.  GPE_ERR_STATE before
 * a gpe_sp_compute that returned 0.  Changes nothing a later gpe_sp_nlml / gpe_sp_predict / gpe_sp_get_* reads. */
int gpe_sp_grad(gpe_sp_handle h, double* d_xb, double* d_hp);
/* spgp.hpp:446-451, one `_likelihood(x, true)`: gpe_sp_set_pseudo (Xb_rowmajor: M x D with the handle's M, or NULL: the
 * pseudo-inputs stay) + gpe_sp_set_hparams + gpe_sp_compute + gpe_sp_nlml + gpe_sp_grad in one call.  nlml: P values; d_xb may be
 * NULL.  Any status other than 0 (a pivot: > 0) leaves nlml, d_xb and d_hp untouched. */
int gpe_sp_objective_grad(gpe_sp_handle h, const double* Xb_rowmajor, const double* log_b, double log_c, double log_sig, double jitter,
                          double* nlml, double* d_xb, double* d_hp);
/* Instrumentation: under gpe_sp_set_profiling(1), the phases of the last gradient in ms, ms5 = { the triangular inverses and
 * the M x M setup, the cross kernel and the two products (all chunks), the per-point and row-sum kernels, TT, the finish }. */
int gpe_sp_grad_phase_ms(gpe_sp_handle h, double* ms5);

#ifdef __cplusplus
}
#endif
#endif /* GPE_SPARSE_GRAD_H */
