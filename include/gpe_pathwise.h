/*
 * gpe_pathwise.h — posterior draws as FUNCTIONS of the query point: pathwise conditioning (Matheron's rule) on a random-Fourier-
 * feature prior (Wilson et al. 2020, "Efficiently sampling functions from Gaussian process posteriors").
 *
 * gpe_joint_draws (gpe_joint.h) draws on a finite candidate set: all M points resident, an M x M covariance and its Cholesky, no
 * value between candidates, no gradient.  A path set is S draws per output that can be evaluated anywhere, any number of times:
 *   f_s(x)  = m(x) + Phi(x) w_s + k(x, X) u_s
 *   u_s     = (K + (noise + 1e-8) I)^-1 (obs_mean - Phi(X) w_s - sqrt(noise + 1e-8) eps_s)
 *   Phi(x)_r = sqrt(2 sf2 / R) cos(omega_r . x + b_r)
 * One multi-right-hand-side solve when the set is made; after that S draws at T points cost O(T N S + T R S): no triangular solve
 * per point, no M x M matrix, no cap on T — and an exact gradient in x:
 *   d f_s / dx = -sum_r sqrt(2 sf2 / R) sin(omega_r . x + b_r) omega_r w_rs + sum_i u_is dk(x, x_i)/dx     (dk/dx: gpe_query_grad.h)
 *
 * Conventions of gpe.h / gpe_joint.h: host pointers, int status, column-major, the caller supplies all randomness.
 *
 * Frequencies.  Dw = D for every kind except SE-ARD with Lambda (k columns), where Dw = D + k.  Omega0 (R x Dw, row-major) holds draws
 * from the kernel family's spectral law at unit length scale: standard normals for SE-ARD and Exp (limbo's Exp is the isotropic
 * squared exponential, gpe_query_grad.h); z sqrt(2 nu / u), u ~ chi^2(2 nu), for Matern-nu (5 degrees of freedom for Matern-5/2, 3 for
 * Matern-3/2).  The engine scales them by the handle's current hyper-parameters: omega_d = Omega0_d / ell_d (SE-ARD; isotropic kinds
 * Omega0 / l), and with Lambda omega = diag(1/ell) Omega0[0 .. D) + Lambda Omega0[D .. D + k): the spectral covariance is then
 * diag(ell^-2) + Lambda Lambda^T, the Mm of gpe_query_grad.h.
 *
 * Semantics.
 *   gpe_paths_create needs a computed model (GPE_ERR_STATE otherwise) and does not change it: gpe_epoch does not move, later queries
 *   and log-likelihoods return the same bits.  The one exception is gpe_query_batch_grad's: below one outer panel (or where the
 *   transposed layout does not serve the model) U = K^-1 R is one product with the engine's K^-1, which the handle then holds cached.
 *   SNAPSHOT: the set owns copies of everything an evaluation needs — X, the kernel kind and its parameters, Omega, the phases, W and
 *   U = [u_s] (N x S P) — and a stream of its own.  gpe_add_sample(s), gpe_set_kernel, gpe_compute on the handle afterwards do not
 *   change its answers, bitwise; it is destroyed independently of the handle.  It lives on the handle's device.
 *   mean_q is m(v) evaluated by the caller (as in gpe_joint_draws); dF does not contain the mean functor's derivative (as the
 *   gradients of gpe_query_batch_grad).  Column c = s + S p of W, E, F is draw s of output p.
 *   status: 0; GPE_ERR_ARG for null required pointers, R < 1, R > 16384, S < 1, S P > 1024, T < 0, values that are not finite;
 *   GPE_ERR_UNSUPPORTED for GPE_KERNEL_HOST_K handles.  T = 0 returns 0 and does nothing.
 *
 * Bitwise contracts: the same call twice gives the same bits (no floating-point atomics; the sums over the features and over the
 * samples run in a fixed order); a point's answers do not depend on the batch it is asked in (tiles and segment counts come from N,
 * R, S P and D alone; thread = point); F alone and dF alone are the full call's bits; T is chunked internally and unbounded.
 */
#ifndef GPE_PATHWISE_H
#define GPE_PATHWISE_H

#include "gpe.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpe_paths_ctx* gpe_paths;

int gpe_paths_create(gpe_handle h, int R, int S,
                     const double* Omega0, /* R x Dw row-major, unit-scale frequencies (above)       */
                     const double* phase,  /* R, in [0, 2 pi)                                        */
                     const double* W,      /* R x S x P, r fastest: W[r + R (s + S p)], std normal   */
                     const double* E,      /* N x S x P, n fastest, std normal (NULL: zeros)         */
                     gpe_paths* out);
int gpe_paths_eval(gpe_paths ps, const double* Xq_rowmajor, int64_t T, const double* mean_q /* T x P or NULL */,
                   double* F,   /* T x S x P or NULL: F[t + T (s + S p)]               */
                   double* dF); /* T x D x S x P or NULL: dF[t + T (d + D (s + S p))]  */
/* the maximiser of every draw over the T points: S x P each; the lowest index on exact ties; F never leaves the device */
int gpe_paths_argmax(gpe_paths ps, const double* Xq_rowmajor, int64_t T, const double* mean_q, int64_t* argmax, double* fmax);
int gpe_paths_info(gpe_paths ps, int64_t* N, int* D, int* P, int* R, int* S);
/* ms: { create: the features at X (with the residual) | create: the solve | last eval / argmax: the feature term | its data term
 * (with the fold) }, the last two summed over the call's chunks */
int gpe_paths_phase_ms(gpe_paths ps, double* ms4);
int gpe_paths_destroy(gpe_paths ps);

#ifdef __cplusplus
}
#endif
#endif /* GPE_PATHWISE_H */
