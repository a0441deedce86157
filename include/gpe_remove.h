/*
 * gpe_remove.h — remove samples from a fitted model by a blocked update of its factor: the missing half of gpe_append.h.
 *
 * gpe_add_sample / gpe_add_samples append rows to L at O(n^2) cost; the reference (src/limbo/model/gp.hpp) has no call that takes a
 * row out, and neither had this engine: forgetting a sample meant gpe_set_data + gpe_compute on what is left, n^3 / 3 flops for a
 * change that touches far less.  A model at its capacity that drops a point for every point it adds, hallucinated observations
 * that are retracted when the real values arrive, outliers found by the leave-one-out scores: all of them remove.
 *
 * For a model of n samples with factor L and the set R of q indices to remove, i0 = min R: sweep the columns c = i0 .. n - 1 of L.
 *   c in R   the part of column c below its diagonal becomes an update vector; row and column c disappear.  No arithmetic.
 *   c kept   the column absorbs the live vectors by an orthogonal transformation chosen from (L[c, c], u_0[c], u_1[c], ...) that
 *            zeroes every u_k[c] and leaves a positive diagonal d' = sqrt(d^2 + sum u_k[c]^2).
 * What remains in the kept rows and columns is the Cholesky factor of K[S, S], S the kept set in its original order; rows and
 * columns below i0 are untouched.  Every step is a POSITIVE rank-1 update: no pivot can fail, the update is backward stable.
 *
 * Semantics.  The model afterwards is what gpe_set_data on the remaining samples in their original order, with the same kernel,
 * followed by gpe_compute, leaves, to rounding: L, alpha, the log-likelihood terms, the sample matrix.  gpe_nb_samples drops by q,
 * gpe_epoch moves, cached K^-1 / leave-one-out state is invalid (as after gpe_add_samples); capacity and the leading dimension do
 * not shrink.  The same call on the same state is bitwise reproducible, and the order of idx does not matter (it is sorted).
 *   idx        q distinct indices in 0 .. N - 1, any order
 *   obs_mean   (N - q) x P, column-major with leading dimension N - q: ALL remaining rows (the data mean changes when rows leave,
 *              so the caller recomputes it, as for gpe_add_samples)
 *   how        GPE_REMOVE_UPDATE: the factor update; GPE_REMOVE_RECOMPUTE: K rebuilt on the remaining samples and factored by the
 *              engine's own schedule; GPE_REMOVE_AUTO: whichever the plan (gpe_debug_remove_plan) expects to be faster
 *   status     0, never a positive value.  GPE_ERR_ARG: null pointers, q < 0, an index outside 0 .. N - 1, a repeated index,
 *              q >= N (emptying a model is the caller's business), P that disagrees with the handle, an unknown `how`;
 *              GPE_ERR_STATE: samples but no factor; GPE_ERR_UNSUPPORTED: GPE_KERNEL_HOST_K handles.  On any error the model is
 *              unchanged.  NaNs already in the factor propagate.
 *   q == 0     returns 0 and changes nothing, the epoch included.
 *
 * How.  At most gpe_remove_max_vectors() update vectors are carried at once; a longer list goes in successive passes over
 * ascending index ranges inside the one call, with one host wait at the end.  A pass writes the new factor into a second
 * ld x cap matrix (the K^-1 slot, which the call invalidates anyway) — head copy, then two launches per 256-column panel of the
 * old factor from the panel that holds i0 (csrc/remove.hip) — and the two matrices change places.  The samples' SoA rows move, the
 * diagonal-block inverses from block i0 / 64 on are refreshed, alpha and the log-likelihood terms follow once.  If R is exactly the
 * last q indices nothing is launched on the factor: the order shrinks, the last block's inverse is refreshed, alpha is solved.
 */
#ifndef GPE_REMOVE_H
#define GPE_REMOVE_H

#include "gpe.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { GPE_REMOVE_AUTO = 0, GPE_REMOVE_UPDATE = 1, GPE_REMOVE_RECOMPUTE = 2 };

int gpe_remove_samples(gpe_handle h, const int64_t* idx, int64_t q,
                       const double* obs_mean /* (N-q) x P, column-major, ld N-q, ALL remaining rows */, int P, int how);
/* update vectors carried per pass: a longer list goes in successive passes inside the one call */
int gpe_remove_max_vectors(void);
/* Test hook, host only: what a call that removes q indices, the smallest of them i0, from a model of n samples does.
 * out4 = { the path AUTO takes (1 update, 2 recompute), passes, launches on the factor, scratch doubles }.  tail_only != 0: the
 * indices are exactly n - q .. n - 1 (then i0 must be n - q).  The launch count of passes behind the first is an upper bound:
 * they start at the pass's own smallest index, which is not below i0.  GPE_ERR_ARG: null out4, n <= 0, q < 0, q >= n,
 * i0 outside 0 .. n - q, a tail_only that contradicts i0. */
int gpe_debug_remove_plan(int64_t n, int64_t i0, int64_t q, int tail_only, int64_t* out4);

#ifdef __cplusplus
}
#endif
#endif /* GPE_REMOVE_H */
