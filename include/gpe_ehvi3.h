/*
 * gpe_ehvi3.h — the exact expected hypervolume improvement of three objectives over a Pareto front.
 *
 * gpe_ehvi.h scores two objectives over the front the user holds; for three the engine had max-value entropy search alone, whose
 * value rests on sampled maxima.  The reference's side of this is src/ehvi (Hupkens' 2-, 5-, 8-term and slice-update schemes), sums
 * whose terms subtract.  Here it is a sum over at most 2n + 1 boxes whose every term is positive (gpe.h conventions: column-major,
 * host pointers, status).
 *
 * Semantics.  All three objectives are MAXIMISED.  ref = (r1, r2, r3) lies strictly below every front point in all three.  A
 * candidate's objectives are independent Gaussians (mu_k, s_k); s are STANDARD DEVIATIONS (gpe_ehvi.h, "Units").
 *   psi_k(t)    E[(Y_k - t)+] = s_k f((mu_k - t) / s_k),  f(z) = phi(z) + z Phi(z);  psi_k(+inf) = 0;  d psi / d mu = Phi, d psi / d s = phi
 *   height      fix a height axis c, the other two a < b.  A point p >= ref is not dominated by the front exactly when
 *               p_c > h_c(p_a, p_b): the largest f_c among the front points that dominate (p_a, p_b) in the plane, r_c if none does.
 *               h_c is piecewise constant on rectangles.
 *   boxes       the front is swept in descending f_c with the staircase of the points seen so far in the (a, b) plane.  A point q
 *               that dominates t points of the staircase newly dominates a region of t + 1 vertical strips, each a rectangle
 *               [l_a, u_a) x [l_b, u_b) of height q_c; the t points leave the staircase.  What lies outside the final staircase of k
 *               points is k + 1 strips of height r_c, unbounded (u = +inf).  Empty rectangles are dropped.  The rectangles are
 *               disjoint and cover [r_a, inf) x [r_b, inf); they are at most 2n + 1, and exactly as many in general position.
 *   ehvi        sum_boxes (psi_a(l_a) - psi_a(u_a)) (psi_b(l_b) - psi_b(u_b)) psi_c(h)              (any c gives the same number)
 *   partials    M x 6, column-major: d/d mu1, d/d s1, d/d mu2, d/d s2, d/d mu3, d/d s3:
 *                 d/d mu_c, d/d s_c = sum_boxes (psi_a(l_a) - psi_a(u_a)) (psi_b(l_b) - psi_b(u_b)) {Phi_c, phi_c}(h)
 *               taken from the table whose height axis is c — three tables; psi falls with t, so every factor and every term of
 *               every sum is >= 0: no Phi(l) - Phi(u) and no phi(l) - phi(u) is formed.  The value is the sum over the table
 *               with c = 3; with partials == NULL that table alone is built and summed.
 *   s_k = 0     psi_k(t) = max(mu_k - t, 0), Phi = [mu_k > t], phi = 0: the limit; with all three zero ehvi is the plain hypervolume
 *               improvement of the point mu.
 *   n = 0       legal: psi_1(r1) psi_2(r2) psi_3(r3).
 *   NaN         a NaN in a candidate's belief gives NaN for that candidate alone.  mu = -inf gives 0; mu = +inf gives +inf or a
 *               finite value, never NaN (0 inf = 0: a box of no expected width under an unbounded height; psi(l) - psi(u) of two
 *               infinite values is the width u - l).  No input makes a loop longer: the steps are counted by the boxes alone.
 *   The model is not changed: gpe_epoch does not move, later queries answer bitwise what they answered before.  The same call on
 *   the same inputs is bitwise reproducible, and a candidate's value and partials are bitwise the same in whatever batch it is asked:
 *   one wave sums a candidate's boxes in an order fixed by the box count alone, never by M; the tile of every product of the solves
 *   comes from N alone (gpe_kg.h); no atomics.
 *
 * Limits.  n <= GPE_EHVI3_MAX_FRONT: one table is at most 2n + 1 boxes of 5 doubles, 82 KB; the kernel stages it through LDS in
 * pieces of a fixed size.  M is unbounded: the candidates stream in chunks.
 *
 * Cost.  The tables: O(n^2) on the host at worst (a sorted staircase; n log n in general position), once per call.  The kernel: M
 * (2n + 1) box steps per table, each five exp + erfc pairs in fp64 on the vector units — three tables with partials, one without;
 * gpe_ehvi3_batch adds gpe_query_batch's solves, 2 M N^2 flops on the matrix cores.
 */
#ifndef GPE_EHVI3_H
#define GPE_EHVI3_H

#include "gpe.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPE_EHVI3_MAX_FRONT 1024

/* Host only, no handle: the front of the n points F (row-major n x 3) above ref3 = (r1, r2, r3).  Keeps the finite points strictly
 * above ref3 in all three objectives, drops dominated points and all duplicates but one, orders descending in f3, ties ascending in
 * f1, then in f2: what the calls below take as `front`.  out_rowmajor has room for n points; *n_out is how many were written.  Any
 * n >= 0; O(n^2) at worst.  GPE_ERR_ARG: a NaN in F or ref3, a ref3 that is not finite, n < 0, a NULL pointer. */
int gpe_ehvi3_front(const double* F_rowmajor, int64_t n, const double* ref3, double* out_rowmajor, int64_t* n_out);

/* Host only, no handle: the table of the prepared front (row-major n x 3) for the height axis `axis` in {0, 1, 2}: rows
 * {l_a, u_a, l_b, u_b, h}, a < b the other two axes, u may be +inf; boxes_rowmajor has room for cap rows (2n + 1 always suffice),
 * *n_boxes is how many were written.  The order of the rows is a function of the front alone (the sweep's).  It is also the
 * prepared-front check, and what the two calls below run first: GPE_ERR_ARG for a front that holds a dominated or duplicate point, a
 * point not above ref3, a value that is not finite, or a wrong order; for n < 0, n > GPE_EHVI3_MAX_FRONT, a ref3 that is not finite,
 * an axis outside {0, 1, 2}, a NULL pointer, and a cap the table does not fit (nothing is written then). */
int gpe_ehvi3_boxes(const double* front_rowmajor, int64_t n, const double* ref3, int axis, double* boxes_rowmajor, int64_t cap,
                    int64_t* n_boxes);

/* The box sums alone on beliefs the caller computed: ehvi[m] and partials (M x 6 column-major, may be NULL) of candidate m with the
 * means mu and standard deviations s (each M x 3 column-major).  Any handle of the device serves, computed or not; serves three
 * independent models, the sparse model, any Gaussian belief.  front: prepared (gpe_ehvi3_front makes one), checked on the host,
 * otherwise GPE_ERR_ARG, as are n < 0, n > GPE_EHVI3_MAX_FRONT, M < 0, a ref3 that is not finite and a negative s (a NaN s is a
 * belief like any other: NaN out).  The front check precedes everything that needs the device: with M = 0 the call IS that check
 * (0 or GPE_ERR_ARG) and does nothing else; h may then be NULL.  GPE_ERR_UNSUPPORTED for GPE_KERNEL_HOST_K handles. */
int gpe_ehvi3_values(gpe_handle h, const double* front_rowmajor, int64_t n, const double* ref3, const double* mu, const double* s,
                     int64_t M, double* ehvi, double* partials);

/* One computed handle with P >= 3 outputs; the objectives are its outputs outs3[0 .. 2], pairwise distinct.  One factorisation and
 * one solve serve all three and they share sigma (limbo's GP with dim_out = 3).  The candidates Xc (row-major M x D) stream through
 * gpe_query_batch's chunk pipeline; the box kernel runs on each chunk's means and variance where they lie, nothing returns to the
 * host in between.
 *   mean_add   M x 3 column-major or NULL: the mean functor's values of the three outputs, added to k^T alpha on the device
 *   s^2        (var > DBL_EPSILON ? var : 0) + var_add — the clamp of gp.hpp:621-623; var_add = 0: the latent function, var_add =
 *              the kernel's noise: the observation;  s1 = s2 = s3 = sqrt(s^2)
 *   partials   M x 6 column-major or NULL, as above (d/d s_k apart: d/d s of the shared sigma is their sum)
 *   mu, var    optional read-backs: mu (M x 3 column-major) = k^T alpha + mean_add of the three outputs; var (M) =
 *              gpe_query_batch's var — no clamp, nothing added
 * Status: GPE_ERR_STATE before gpe_compute; GPE_ERR_UNSUPPORTED for GPE_KERNEL_HOST_K handles; GPE_ERR_ARG for outputs that are not
 * pairwise distinct or outside [0, P), a NULL outs3, a bad front (as above), M < 0, a var_add that is negative or not finite.  The
 * front check (the tables, built on the host) comes first, then the handle's state, then its kernel, then the outputs: a bad front is
 * GPE_ERR_ARG whatever the handle's state, also with M = 0.  On an error no output is written.  M = 0 is otherwise a no-op. */
int gpe_ehvi3_batch(gpe_handle h, const int* outs3, const double* Xc_rowmajor, int64_t M, const double* mean_add, double var_add,
                    const double* front_rowmajor, int64_t n, const double* ref3, double* ehvi, double* partials, double* mu, double* var);

/* Instrumentation: while gpe_set_profiling is on, the phases of the handle's last gpe_ehvi3_batch in ms — { the solves (head, solve,
 * variance); the box kernel; the read-back }, summed over the chunks. */
int gpe_ehvi3_phase_ms(gpe_handle h, double* ms3);

#ifdef __cplusplus
}
#endif
#endif /* GPE_EHVI3_H */
