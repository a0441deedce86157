// append.hpp — a batch of samples appended to a fitted model in one blocked update (include/gpe_append.h): host side.
// Kernels: append.hip (the tail), gemm.hip / kbuild.hip / inv.hip through the chunk helpers of query.hpp (the solve).
// A part of engine.hip's translation unit (included there, once, behind query.hpp, whose chunk helpers it shares).
#pragma once

// The launch list of one chunk of mc <= append_max_chunk() points on a factor of order n ("Blocked append"):
//   chunk_begin               1   inverses of the 256-column diagonal panels (inv.hip)
//   chunk_head, chunk_solve   3 + 2 ceil(n / 256) - 1: points to SoA (+ Lambda rows), cross kernel, then per panel the product
//                             with the panel inverse and the update of what lies right of it — Zt = Kst L^-T on the matrix cores
//   copy2d                    1   the points' SoA columns n .. n + mc - 1 of Xt (they are SoA already: no second transposition)
//   launch_append_tail        3   partial products + rows of L | fold + k(V, V) | factorisation + C + pivot word (append.hip)
//   launch_diag_inv           1   EVERY 64-block that gained rows, the partly old first one included
// and once per call, behind the last chunk: solve_alpha (two sweeps), the log-likelihood terms, compute_finish (the one host wait).
// (extra: the tail's scratch in front of the chunk buffers in dQuery, slices_cap partial matrices and S — sized by the caller for
// the largest order the call reaches, append_scratch_doubles(nb0 + rem))
// The call's scratch: the tail's, then a chunk's buffers — reserved once for the last chunk's layout, placed per chunk for its own
static void append_regions(Carver& cv, size_t extra, QtBufs& b)
{
    cv.take<double>(extra);
    qt_carve(b, cv);
}
static int append_enqueue(gpe_ctx* c, const double* Xb, int64_t nb0, int64_t rem, size_t extra, int slices_cap)
{
    hipStream_t s = c->stream;
    const int64_t ld = c->ld, CH = append_max_chunk();
    c->N = nb0;
    for (int64_t m0 = 0; m0 < rem; m0 += CH) {
        const int64_t mc = std::min<int64_t>(CH, rem - m0), n = c->N;
        QtBufs b = qt_layout(c, CH, n); // (the chunk in front of this one is part of L by now)
        Carver cv(c->dQuery.get());
        append_regions(cv, extra, b);
        chunk_begin(c, b, true);
        chunk_head(c, b, Xb + m0 * c->D, true, mc, true, false, nullptr, 0, 0);
        chunk_solve(c, b, mc);
        {
            PhaseScope ps(c, GPE_PH_POTRF_PANEL, (double)mc * mc * n + (double)mc * mc * mc / 3.0);
            launch_copy2d(s, b.dQt, b.ldq, c->dXt + n, ld, mc, c->kp.D);
            if (!launch_append_tail(s, b.dZt, b.dQt, b.ldq, (int)mc, n, c->kp, c->dA, ld, c->dInfo, c->dQuery, slices_cap)) {
                c->err = "add_samples: the tail's scratch was not sized for this chunk";
                return GPE_ERR_STATE;
            }
            launch_diag_inv(s, c->dA, ld, n + mc, n / NB, (n + mc - 1) / NB - n / NB + 1, c->dXinv);
        }
        c->N = n + mc;
    }
    c->have_L = true;
    c->inv_ok = false; // gp.hpp:602
    solve_alpha(c);    // gp.hpp:599, once
    enqueue_loglik_terms(c);
    return GPE_OK;
}

int gpe_append_max_chunk(void) { return append_max_chunk(); }

int gpe_debug_append_slices(int64_t n, int64_t* kslice, int* nslices, int* slices_cap, int64_t* scratch_doubles)
{
    if (n < 0)
        return GPE_ERR_ARG;
    int64_t ks;
    int nsl;
    append_slices(n, &ks, &nsl);
    if (kslice)
        *kslice = ks;
    if (nslices)
        *nslices = nsl;
    if (slices_cap)
        *slices_cap = append_slices_cap(n);
    if (scratch_doubles)
        *scratch_doubles = (int64_t)append_scratch_doubles(n);
    return GPE_OK;
}

int gpe_add_samples(gpe_handle c, const double* X, int64_t q, int D, const double* obs_mean, int P)
{
    if (!c || q < 0)
        return GPE_ERR_ARG;
    if (q == 0)
        return GPE_OK;
    ++c->epoch;
    if (!X || !obs_mean || D <= 0 || P <= 0)
        return GPE_ERR_ARG;
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->host_K)
        return GPE_ERR_UNSUPPORTED;
    const int64_t n0 = c->N, nfin = n0 + q;
    if (n0 == 0) { // gp.hpp:128-137
        if (D > GPE_MAX_THETA - 2)
            return GPE_ERR_ARG;
    }
    else {
        if (D != c->D || P != c->P) // gp.hpp:139-140
            return GPE_ERR_ARG;
        if (!c->have_L)
            return GPE_ERR_STATE;
    }
    if (lam_columns(c->kind, c->n_theta, D) < 0) {
        c->err = "set_kernel: wrong number of hyper-parameters for this kernel/dimension";
        return GPE_ERR_ARG;
    }
    // capacity once for the whole batch
    if (n0 == 0) {
        const int rc = alloc_dev(c, std::max<int64_t>(256, nfin), D, P);
        if (rc)
            return rc;
        c->D = D;
        c->P = P;
    }
    else {
        const int rc = grow_dev(c, nfin);
        if (rc)
            return rc;
    }
    // Point by point — gpe_add_sample's launches AND its host wait per point (one launch and a spin on a pinned word on the small
    // path, the three sweeps and a stream wait above it) — while the model has less than one outer panel (the transposed solve
    // needs one) and when the whole append stays inside the one-launch small path
    const bool small_all = c->small_path && nfin <= small_max_n() && P <= 3;
    int status = 0;
    int64_t done = 0;
    while (done < q && (small_all || !qt_serves(c))) {
        const int rc = add_sample_locked(c, X + done * D, D, obs_mean, nfin, P, n0 == 0 && done == 0);
        if (rc < 0)
            return rc;
        if (rc > 0 && status == 0)
            status = rc;
        ++done;
    }
    if (done == q)
        return status;
    // the rest as a block: chunks of <= append_max_chunk() rows, one stream, no host wait before compute_finish
    hipStream_t s = c->stream;
    const int64_t nb0 = c->N, rem = q - done;
    const double* Xb = X + done * D;
    digest_kernel(c);
    // scratch once, for the largest order any chunk of the call sees (the slice count of the tail is NOT monotone in n above
    // 65 536 samples: append_slices_cap) and the chunk buffers of the last chunk's layout, which grows with n
    const int slices_cap = append_slices_cap(nfin);
    const size_t extra = append_scratch_doubles(nfin);
    QtBufs blast = qt_layout(c, append_max_chunk(), nfin, nfin);
    QueryScratch qs(c);
    if (const int e = qs.carve([&](Carver& cv) { append_regions(cv, extra, blast); }))
        return e;
    HIPCHK(c, copy2d_from_host(c->dOm, c->ld, obs_mean, nfin, nfin, P, s));
    c->hInfo[0] = c->hInfo[1] = 0; // nothing of this handle is in flight here
    {
        const int e = append_enqueue(c, Xb, nb0, rem, extra, slices_cap);
        if (e)
            return e;
    }
    const int rc = compute_finish(c, [c, Xb, nb0, rem, extra, slices_cap] {
        c->hInfo[0] = 0; // (the re-run repeats the solve, the tail and the sweeps from the untouched inputs)
        (void)append_enqueue(c, Xb, nb0, rem, extra, slices_cap);
    });
    if (rc < 0)
        return rc;
    return status != 0 ? status : rc;
}
