/*
 * gpe_append.h — append a BATCH of samples to a fitted model in one blocked update.
 *
 * gpe_add_sample (gpe.h) is limbo::model::GP::add_sample's incremental Cholesky (src/limbo/model/gp.hpp:126-152, 573-603): one
 * forward substitution for the new row and a complete alpha re-solve per point.  A batch-acquisition loop (acqui/thompson.hpp:
 * propose q points, evaluate them, add them, ask again) brings q observations back at once; the call below applies gp.hpp:583-597
 * to the block.  The reference has no such call; it rests on the same lines and keeps their conventions (gpe.h: column-major,
 * host pointers, status).
 *
 * For a model of n samples with factor L, kernel k and q new points V (row-major q x D):
 *   Z     = L^-1 k(X, V)                                  n x q, the kernel WITHOUT noise (the indices differ)
 *   C     = chol( k(V, V) + (noise + 1e-8) I - Z^T Z )    q x q lower; + noise + 1e-8 on the diagonal only (kernel/kernel.hpp:83):
 *                                                         off-diagonal entries carry none, even between coincident points, as
 *                                                         with successive gpe_add_sample calls
 *   L_new = [ L 0 ; Z^T C ],   alpha = L_new^-T L_new^-1 obs_mean       (gp.hpp:599, 605-611), ONCE
 *
 * Semantics.  The model afterwards is what q successive gpe_add_sample calls with the same points in order — each with the leading
 * rows of the same obs_mean — would leave, to rounding (not bitwise): L, alpha, the log-likelihood terms, the sample matrix.
 * gpe_nb_samples grows by q, gpe_epoch moves, cached K^-1 / leave-one-out state is invalid (gp.hpp:602).  The same call on the
 * same state is bitwise reproducible.
 *   obs_mean   (N + q) x P, column-major with leading dimension N + q: ALL rows, as for gpe_add_sample
 *   status     0; > 0: the 1-based index, in the whole matrix, of the first non-positive pivot — all q samples are appended and
 *              NaNs propagate from that row, as with the single call; a later gpe_compute recovers.
 *              GPE_ERR_ARG: q < 0, null pointers, D or P that disagree with the handle, a hyper-parameter count that does not fit;
 *              GPE_ERR_STATE: samples but no factor; GPE_ERR_UNSUPPORTED: GPE_KERNEL_HOST_K handles.
 *   q == 0     returns 0 and changes nothing, the epoch included.
 *   An empty handle works as with gpe_add_sample.
 *
 * How.  With at least one 256-column outer panel of samples the batch goes in chunks of <= gpe_append_max_chunk() rows: the
 * solve Zt = (L^-1 k(X, V))^T is the batched query's matrix-core product (the same launches), the Schur complement, its
 * factorisation and the new rows of L are three launches more (csrc/append.hip), the diagonal-block inverses of every 64-block that
 * gained rows are refreshed, and alpha and the log-likelihood terms follow once, after the last chunk: the factor is read about
 * three times per chunk-and-call instead of three times per point, and the host waits once.  Below one outer panel — and while the
 * whole append stays inside the one-launch small path — the points are appended inside the one call by gpe_add_sample's own
 * launches, WITH its host wait per point: one launch and a spin on a pinned word each on the small path (P <= 3), the row, alpha's
 * two sweeps and a stream wait each above it (P > 3, or the small path disabled) — up to 255 points before the block path takes over.
 * Capacity grows once, to at least n + q.
 */
#ifndef GPE_APPEND_H
#define GPE_APPEND_H

#include "gpe.h"

#ifdef __cplusplus
extern "C" {
#endif

int gpe_add_samples(gpe_handle h, const double* Xnew_rowmajor, int64_t q, int D,
                    const double* obs_mean /* (N+q) x P, column-major, ALL rows */, int P);
/* rows the device tail factorises at once: a longer batch is processed as successive chunks inside the one call */
int gpe_append_max_chunk(void);
/* Test hook, host only: how the tail splits the k range (length n) of one chunk's product Zt Zt^T over workgroups — slices of
 * kslice columns, nslices of them, each with a partial matrix of gpe_append_max_chunk()^2 doubles — and what a call whose chunks
 * see orders up to n reserves: slices_cap partial matrices and S, scratch_doubles in all.  nslices is not monotone in n above
 * 65 536 samples; slices_cap(n) >= nslices(n') for every n' <= n.  Any output may be null.  GPE_ERR_ARG for n < 0. */
int gpe_debug_append_slices(int64_t n, int64_t* kslice, int* nslices, int* slices_cap, int64_t* scratch_doubles);

#ifdef __cplusplus
}
#endif
#endif /* GPE_APPEND_H */
