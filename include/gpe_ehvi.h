/*
 * gpe_ehvi.h — the exact expected hypervolume improvement of two objectives over a Pareto front.
 *
 * Every other acquisition of the engine scores one objective.  With two, the value of a candidate is the expected growth of the area
 * its outcome adds to what the front already dominates.  The reference's side of this is experimental (experimental/acqui/ehvi.hpp,
 * src/ehvi): a walk over O(n^2) grid cells that subtracts two products per cell.  Here it is an O(n) sum over strips whose every
 * term is positive (gpe.h conventions: column-major, host pointers, status).
 *
 * Semantics.  Both objectives are MAXIMISED.  The front y(1) .. y(n) is sorted ascending in f1, hence strictly descending in f2;
 * ref = (r1, r2) lies strictly below every front point in both.  A candidate's two objectives are independent Gaussians (mu1, s1),
 * (mu2, s2); s are STANDARD DEVIATIONS.
 *   psi_k(t)    E[(Y_k - t)+] = s_k f((mu_k - t) / s_k),  f(z) = phi(z) + z Phi(z);  d psi / d mu = Phi(z), d psi / d s = phi(z)
 *   strips      i = 0 .. n:  l_0 = r1, l_i = y1(i);  l_(n+1) = +inf (psi_1 = 0);  h_i = y2(i+1), h_n = r2, psi_2(h_(-1)) = 0
 *   ehvi        sum_i (psi_1(l_i) - psi_1(l_(i+1))) psi_2(h_i)                     strip i: l_i <= f1 < l_(i+1), the front at h_i
 *   partials    M x 4, column-major: d/d mu1, d/d s1, d/d mu2, d/d s2:
 *                 d/d mu2, d/d s2 = sum_i (psi_1(l_i) - psi_1(l_(i+1))) {Phi_2, phi_2}(h_i)
 *                 d/d mu1, d/d s1 = sum_i {Phi_1, phi_1}(l_i) (psi_2(h_i) - psi_2(h_(i-1)))   (the same sum, by parts)
 *               psi is decreasing in t, l ascends and h descends: every term of every sum is >= 0; nothing like the reference's
 *               psi1 psi2 - S gausscdf1 gausscdf2 is formed.
 *   s_k = 0     psi_k(t) = max(mu_k - t, 0), Phi = [mu_k > t], phi = 0: the limit; with s1 = s2 = 0 ehvi is the plain hypervolume
 *               improvement of the point (mu1, mu2).
 *   NaN         a NaN in a candidate's belief gives NaN for that candidate alone.  mu = +inf gives +inf or a finite value, mu = -inf
 *               gives 0; no input makes a loop longer than n + 2 steps.
 *   n = 0       legal: psi_1(r1) psi_2(r2), the product of two one-sided expected improvements.
 *   The model is not changed: gpe_epoch does not move, later queries answer bitwise what they answered before.  The same call on
 *   the same inputs is bitwise reproducible, and a candidate's value and partials are bitwise the same in whatever batch it is asked:
 *   one wave sums a candidate's strips in an order fixed by n alone, never by M; the tile of every product of the solves comes
 *   from N alone (gpe_kg.h); no atomics.
 *
 * Units.  The reference's acquisition hands model.sigma(v) — a VARIANCE, the kernel's noise added (model/gp.hpp:186-191) — to the
 * slot where its ehvi2d expects a standard deviation (experimental/acqui/ehvi.hpp:76).  That is not reproduced: s here is
 * sqrt(variance), and whether the noise is in the variance is the caller's choice (var_add).
 *
 * Limits.  n <= GPE_EHVI_MAX_FRONT: the front sits in one workgroup's LDS (32 KiB).  M is unbounded: the candidates stream in chunks.
 *
 * Cost.  M (n + 2) strip steps, each two exp + erfc pairs in fp64 on the vector units (f, Phi and phi at l_i and at h_i; the
 * neighbours' values come across lanes); gpe_ehvi2_batch adds gpe_query_batch's solves, 2 M N^2 flops on the matrix cores.
 */
#ifndef GPE_EHVI_H
#define GPE_EHVI_H

#include "gpe.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPE_EHVI_MAX_FRONT 2048

/* Host only, no handle: the front of the n points F (row-major n x 2) above ref2 = (r1, r2).  Keeps the finite points with
 * f1 > r1 and f2 > r2, drops dominated points and all duplicates but one, sorts ascending in f1: what the calls below take as
 * `front`.  out_rowmajor has room for n points; *n_out is how many were written.  Any n >= 0; O(n log n).  GPE_ERR_ARG: a NaN in F
 * or ref2, a ref2 that is not finite, n < 0, a NULL pointer. */
int gpe_ehvi2_front(const double* F_rowmajor, int64_t n, const double* ref2, double* out_rowmajor, int64_t* n_out);

/* The strip sums alone on beliefs the caller computed: ehvi[m] and partials (M x 4 column-major, may be NULL) of candidate m with
 * (mu1[m], s1[m]), (mu2[m], s2[m]).  Any handle of the device serves, computed or not; serves two independent models, the sparse
 * model, any Gaussian belief.  front: row-major n x 2, prepared — strictly ascending f1, strictly descending f2, finite, all above
 * ref2 in both; checked on the host in O(n), otherwise GPE_ERR_ARG, as are n < 0, n > GPE_EHVI_MAX_FRONT, M < 0, a ref2 that is
 * not finite and a negative s (a NaN s is a belief like any other: NaN out).  The front check precedes everything that needs the
 * device: with M = 0 the call IS that check (0 or GPE_ERR_ARG) and does nothing else; h may then be NULL.
 * GPE_ERR_UNSUPPORTED for GPE_KERNEL_HOST_K handles. */
int gpe_ehvi2_values(gpe_handle h, const double* front_rowmajor, int64_t n, const double* ref2, const double* mu1, const double* s1,
                     const double* mu2, const double* s2, int64_t M, double* ehvi, double* partials);

/* One computed handle with P >= 2 outputs; the objectives are its outputs out1 != out2.  One factorisation and one solve serve both
 * and they share sigma (limbo's GP with dim_out = 2).  The candidates Xc (row-major M x D) stream through gpe_query_batch's chunk
 * pipeline; the strip kernel runs on each chunk's means and variance where they lie, nothing returns to the host in between.
 *   mean_add   M x 2 column-major or NULL: the mean functor's values of (out1, out2), added to k^T alpha on the device
 *   s^2        (var > DBL_EPSILON ? var : 0) + var_add — the clamp of gp.hpp:621-623; var_add = 0: the latent function, var_add =
 *              the kernel's noise: the observation;  s1 = s2 = sqrt(s^2)
 *   partials   M x 4 column-major or NULL, as above (d/d s1 and d/d s2 apart: d/d s of the shared sigma is their sum)
 *   mu, var    optional read-backs: mu (M x 2 column-major) = k^T alpha + mean_add of (out1, out2); var (M) = gpe_query_batch's
 *              var — no clamp, nothing added
 * Status: GPE_ERR_STATE before gpe_compute; GPE_ERR_UNSUPPORTED for GPE_KERNEL_HOST_K handles; GPE_ERR_ARG for out1 == out2, an
 * output outside [0, P), a bad front (as above), M < 0, a var_add that is negative or not finite.  M = 0 is a no-op. */
int gpe_ehvi2_batch(gpe_handle h, int out1, int out2, const double* Xc_rowmajor, int64_t M, const double* mean_add, double var_add,
                    const double* front_rowmajor, int64_t n, const double* ref2, double* ehvi, double* partials, double* mu, double* var);

/* Instrumentation: while gpe_set_profiling is on, the phases of the handle's last gpe_ehvi2_batch in ms — { the solves (head, solve,
 * variance); the strip kernel; the read-back }, summed over the chunks. */
int gpe_ehvi_phase_ms(gpe_handle h, double* ms3);

#ifdef __cplusplus
}
#endif
#endif /* GPE_EHVI_H */
