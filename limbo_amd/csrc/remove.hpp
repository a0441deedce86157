// remove.hpp — samples removed from a fitted model by a blocked update of its factor (include/gpe_remove.h): host side.
// Kernels: remove.hip.  A part of engine.hip's translation unit (included there, once, behind append.hpp).
#pragma once

// The launch list of a call that removes q indices (sorted; i0 the smallest) from a factor of order n ("Blocked removal"):
//   launch_rm_xt              1   the SoA rows of the samples (the Lambda^T x rows included) move, in place, one workgroup per row
//   per pass of <= GPE_RM_CAP indices, from the current factor into the other ld x cap matrix (the K^-1 slot):
//     launch_rm_head          1   columns in front of the panel that holds the pass's first index (none if that is panel 0)
//     launch_rm_panel         2   per 256-column panel from there on (1 for the last: no rows below it)
//   memsets                       what lies beyond the new order reads as on a handle that never held more
//   launch_diag_inv           1   every 64-block from i0 / 64 on: all of them shifted
// and once per call: solve_alpha (two sweeps), the log-likelihood terms, compute_finish (the one host wait).
// A tail-only removal (the indices are n - q .. n - 1) launches nothing on the factor.

struct RmPlan {
    int path;         // GPE_REMOVE_UPDATE / GPE_REMOVE_RECOMPUTE: what AUTO takes
    int64_t passes;   // of the update
    int64_t launches; // of the update on the factor (head + panels; an upper bound behind the first pass)
    int64_t scratch;  // doubles
    double upd_us, rec_us; // the rule's two sides
};

// AUTO's rule, fitted to profiles/remove_samples_timing.json, microseconds on an MI355X:
//   update     100 + 0.045 n'                      the samples' rows, the pads, the block inverses, alpha (what a tail-only call costs)
//              + per panel 160 + 9.6 A             k_rm_rot's column-to-column chain: 256 sequential reflectors, A the pass's vector
//                                                  count rounded up to an instantiation (1, 4, 8, 16, 32) — the term that decides
//              + 16 bytes per trailing element at 1.5 TB/s (the apply launches) and per head element at 2.5 TB/s (the copy)
//   recompute  120 + 0.17 n' + 6.5e-9 n'^3         the engine's factorisation at the remaining order n' (0.30 / 1.26 / 31.5 ms at
//                                                  1024 / 4096 / 16 384)
// From index 0 with one vector the two cross near n = 10 000; with 32 vectors near 16 384; a removal whose first index lies in
// the last panels is an update at every order, and a tail-only one always.
static RmPlan rm_plan(int64_t n, int64_t i0, int64_t q, bool tail_only)
{
    const int64_t CAP = GPE_RM_CAP, PW = GPE_RM_PANEL;
    RmPlan pl{};
    pl.scratch = (int64_t)(remove_u_ld(n) * (size_t)CAP + remove_coef_doubles()) + (n + 1) / 2;
    const double nr = (double)(n - q);
    pl.rec_us = 120.0 + 0.17 * nr + 6.5e-9 * nr * nr * nr;
    pl.upd_us = 100.0 + 0.045 * nr;
    if (tail_only || q == 0) {
        pl.path = GPE_REMOVE_UPDATE;
        return pl;
    }
    pl.passes = (q + CAP - 1) / CAP;
    for (int64_t j = 0; j < pl.passes; ++j) {
        const int64_t nj = n - j * CAP, a = std::min<int64_t>(CAP, q - j * CAP);
        const int64_t p0 = std::min(i0, nj - 1) / PW, panels = (nj + PW - 1) / PW - p0;
        pl.launches += (p0 > 0 ? 1 : 0) + 2 * panels - 1;
        const double A = a <= 1 ? 1.0 : a <= 4 ? 4.0 : a <= 8 ? 8.0 : a <= 16 ? 16.0 : 32.0;
        const double ch = (double)(p0 * PW), m = (double)nj - ch;
        pl.upd_us += (double)panels * (160.0 + 9.6 * A) + m * (m + 1.0) * 0.5 * 16.0 / 1.5e6 + ch * ((double)nj - 0.5 * ch) * 16.0 / 2.5e6;
    }
    pl.path = pl.upd_us <= pl.rec_us ? GPE_REMOVE_UPDATE : GPE_REMOVE_RECOMPUTE;
    return pl;
}

int gpe_remove_max_vectors(void) { return remove_max_vectors(); }

int gpe_debug_remove_plan(int64_t n, int64_t i0, int64_t q, int tail_only, int64_t* out4)
{
    if (!out4 || n <= 0 || q < 0 || q >= n || i0 < 0 || i0 > n - q || (q > 0 && i0 >= n))
        return GPE_ERR_ARG;
    if (tail_only && q > 0 && i0 != n - q)
        return GPE_ERR_ARG;
    const RmPlan pl = rm_plan(n, i0, q, tail_only != 0);
    out4[0] = pl.path;
    out4[1] = pl.passes;
    out4[2] = pl.launches;
    out4[3] = pl.scratch;
    return GPE_OK;
}

struct RmScratch {
    double* U = nullptr;
    double* coef = nullptr;
    int* keep = nullptr;
};
static void remove_regions(Carver& cv, int64_t n, RmScratch& r)
{
    r.U = cv.take<double>(remove_u_ld(n) * (size_t)GPE_RM_CAP);
    r.coef = cv.take<double>(remove_coef_doubles());
    r.keep = cv.take<int>((size_t)n);
}

// the passes of the update, from c->dA (order n) into `other` and back in turn; returns true if the result lies in `other`
static bool remove_passes(gpe_ctx* c, const std::vector<int64_t>& R, int64_t n, double* other, const RmScratch& rs)
{
    hipStream_t s = c->stream;
    const int64_t ld = c->ld, CAP = GPE_RM_CAP, PW = GPE_RM_PANEL, ldu = (int64_t)remove_u_ld(n);
    double* src = c->dA;
    double* dst = other;
    int64_t nj = n;
    for (size_t k0 = 0; k0 < R.size(); k0 += CAP) {
        RmList L{};
        L.a = (int)std::min<size_t>(CAP, R.size() - k0);
        for (int k = 0; k < L.a; ++k)
            L.idx[k] = (int)(R[k0 + k] - (int64_t)k0); // (the k0 smaller indices are gone from this pass's source)
        const int64_t ch = L.idx[0] / PW * PW;
        if (ch > 0) {
            PhaseScope ps(c, GPE_PH_POTRF_UPDATE, 0.0);
            launch_rm_head(s, src, dst, ld, nj, ch, L);
        }
        for (int64_t c0 = ch; c0 < nj; c0 += PW) {
            PhaseScope ps(c, GPE_PH_POTRF_UPDATE, (double)(nj - c0) * (double)std::min(PW, nj - c0) * (4.0 * L.a + 4.0));
            launch_rm_panel(s, src, dst, ld, nj, c0, L, c0 == ch, rs.U, ldu, rs.coef);
        }
        nj -= L.a;
        std::swap(src, dst);
    }
    return src == other;
}

static int remove_enqueue_tail(gpe_ctx* c, int64_t i0)
{
    launch_diag_inv(c->stream, c->dA, c->ld, c->N, i0 / NB, (c->N - 1) / NB - i0 / NB + 1, c->dXinv);
    c->have_L = true;
    c->inv_ok = false;
    solve_alpha(c);
    enqueue_loglik_terms(c);
    return GPE_OK;
}

int gpe_remove_samples(gpe_handle c, const int64_t* idx, int64_t q, const double* obs_mean, int P, int how)
{
    if (!c || q < 0)
        return GPE_ERR_ARG;
    if (q == 0)
        return GPE_OK;
    if (!idx || !obs_mean || how < GPE_REMOVE_AUTO || how > GPE_REMOVE_RECOMPUTE)
        return GPE_ERR_ARG;
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->host_K)
        return GPE_ERR_UNSUPPORTED;
    const int64_t n = c->N, nn = n - q;
    if (P != c->P || q >= n)
        return GPE_ERR_ARG;
    std::vector<int64_t> R(idx, idx + q);
    std::sort(R.begin(), R.end());
    if (R.front() < 0 || R.back() >= n || std::adjacent_find(R.begin(), R.end()) != R.end())
        return GPE_ERR_ARG;
    if (!c->have_L)
        return GPE_ERR_STATE;
    if (lam_columns(c->kind, c->n_theta, c->D) < 0) {
        c->err = "set_kernel: wrong number of hyper-parameters for this kernel/dimension";
        return GPE_ERR_ARG;
    }
    const int64_t i0 = R.front();
    const bool tail_only = i0 == nn;
    const RmPlan pl = rm_plan(n, i0, q, tail_only);
    const bool update = how == GPE_REMOVE_UPDATE || (how == GPE_REMOVE_AUTO && pl.path == GPE_REMOVE_UPDATE);
    // everything that can fail for want of memory, in front of the first change
    hipStream_t s = c->stream;
    const int64_t ld = c->ld;
    RmScratch rs;
    QueryScratch qs(c);
    if (const int e = qs.carve([&](Carver& cv) { remove_regions(cv, n, rs); }))
        return e;
    if (update && !tail_only)
        if (const int e = reserve_mat(c, c->dKinv))
            return e;
    ++c->epoch;
    digest_kernel(c);
    c->hInfo[0] = c->hInfo[1] = 0; // nothing of this handle is in flight here
    if (!tail_only) {
        std::vector<int> keep((size_t)nn);
        for (int64_t j = 0, r = 0, k = 0; r < n; ++r) {
            if (k < q && R[k] == r)
                ++k;
            else
                keep[j++] = (int)r;
        }
        HIPCHK(c, hipMemcpyAsync(rs.keep, keep.data(), sizeof(int) * (size_t)nn, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipStreamSynchronize(s)); // (the list is a local)
        launch_rm_xt(s, c->dXt, ld, xt_rows(c->D), rs.keep, nn, n);
    }
    else
        HIPCHK(c, hipMemset2DAsync(c->dXt + nn, sizeof(double) * (size_t)ld, 0, sizeof(double) * (size_t)q, (size_t)xt_rows(c->D), s));
    HIPCHK(c, copy2d_from_host(c->dOm, ld, obs_mean, nn, nn, P, s));
    // the diagonal-block inverses of blocks the model no longer reaches: as alloc_dev left them
    const int64_t nb_new = (nn + NB - 1) / NB, nb_old = (n + NB - 1) / NB;
    if (nb_old > nb_new)
        HIPCHK(c, hipMemsetAsync(c->dXinv + nb_new * NB * NB, 0, sizeof(double) * (size_t)((nb_old - nb_new) * NB * NB), s));
    c->inv_ok = false;
    c->inv_pad_n = -1;
    c->ll_ok = false;
    if (!update) {
        c->N = nn;
        c->have_L = false;
        const int e = compute_enqueue(c);
        if (e)
            return e;
        const int rc = compute_finish(c);
        return rc < 0 ? rc : GPE_OK; // (a principal submatrix of a matrix that was factored)
    }
    if (!tail_only) {
        if (remove_passes(c, R, n, c->dKinv, rs))
            c->dA.swap(c->dKinv);
    }
    // rows and columns [nn, n) of the live factor, the obs_mean^T rows under the old order included: zero, and below the new
    // order whatever the other matrix held there
    {
        const int64_t r1 = std::min(ld, round_up(n, NB) + NB), c1 = std::min(c->cap, round_up(n, NB));
        HIPCHK(c, hipMemset2DAsync(c->dA + nn, sizeof(double) * (size_t)ld, 0, sizeof(double) * (size_t)(r1 - nn), (size_t)nn, s));
        if (c1 > nn)
            HIPCHK(c, hipMemsetAsync(c->dA + nn * ld, 0, sizeof(double) * (size_t)((c1 - nn) * ld), s));
    }
    c->N = nn;
    remove_enqueue_tail(c, tail_only ? nn - 1 : i0);
    const int rc = compute_finish(c);
    return rc < 0 ? rc : GPE_OK;
}
