// joint.hpp — the joint posterior over a point batch (include/gpe_joint.h): host side.  Kernels: joint.hip, gemm.hip (k_gemm_items).
// A part of engine.hip's translation unit (included there, once, behind query.hpp, whose chunk helpers it shares).
#pragma once

// M above this is GPE_ERR_ARG: all M rows of Zt are resident at once (one chunk of the batched query), and Sigma, its factor and
// the partial matrices of the split are M x M each
static int64_t joint_max_points(const gpe_ctx* c)
{
    return qt_rows_per_chunk(c->N, 16384);
}

// The private scratch context that owns Sigma and factors it.  potrf_blocked takes the matrix as an argument but the leading
// dimension, the diagonal-block inverses, the pivot word and the hand-over buffers of the data-flow launches from the context:
// run on the model's own context it would overwrite the dXinv every later query of the model reads.  So Sigma lives in a
// context of its own — kernel kind "K is given" (as after gpe_set_K_host: Sigma is written into its dKhost by the covariance
// kernels, compute_enqueue copies it under the factor, so Sigma survives a failed factorisation), one all-zero right-hand side
// (the engine requires P >= 1), D = 1 — created lazily on the model's device, re-used while M fits, freed with the handle, never
// cloned.  Its evaluations go through compute_enqueue / compute_finish like anybody's: the same gate, lock scopes and re-runs.
// (shared with the sparse model's scratch, sparse.hpp) a dense context shaped for order M and P right-hand sides with the kernel
// kind "K is given" and room for that K; *fresh: its buffers are new, nothing of an earlier order is in them
static int scratch_with_K(gpe_ctx* sc, int64_t M, int P, bool* fresh)
{
    *fresh = M > sc->cap || P != sc->P || !sc->dA || !sc->dKhost;
    if (*fresh) {
        int rc = alloc_dev(sc, M, 1, P);
        if (rc == GPE_OK)
            rc = reserve_mat(sc, sc->dKhost);
        if (rc)
            return rc;
        sc->D = 1;
        sc->P = P;
    }
    sc->N = M;
    sc->kind = GPE_KERNEL_HOST_K;
    sc->host_K = true;
    sc->have_L = sc->inv_ok = sc->ll_ok = false;
    sc->prof = false;
    return GPE_OK;
}
static int joint_scratch(gpe_ctx* c, int64_t M, gpe_ctx** out)
{
    if (!c->joint) {
        gpe_ctx* sc = nullptr;
        const int rc = gpe_create(c->ldevice, &sc);
        if (rc)
            return rc;
        sc->small_path = false;
        c->joint = sc;
    }
    gpe_ctx* sc = c->joint;
    bool fresh = false;
    if (scratch_with_K(sc, M, 1, &fresh) != GPE_OK) {
        c->err = "joint posterior: " + sc->err;
        return GPE_ERR_NOMEM;
    }
    if (fresh) { // the one all-zero right-hand side
        HIPCHK(c, hipMemsetAsync(sc->dOm, 0, sizeof(double) * (size_t)sc->ld, sc->stream));
        HIPCHK(c, hipStreamSynchronize(sc->stream));
    }
    *out = sc;
    return GPE_OK;
}

// Which covariance path: GPE_JOINT_SPLITK=0 the composed one, =1 the split kernel, unset: the split kernel while the lower
// 128 x 128 tiles of Sigma are fewer than two per CU — where a launch of whole tiles leaves the chip idle.  Measured
// (profiles/joint_posterior_timing.json, Sigma phase, split against composed): 0.157 / 0.557 ms at (N, M) = (4096, 512),
// 0.508 / 0.585 at (4096, 2048), 0.553 / 2.136 at (16384, 1024), and 6.70 / 6.07 at (16384, 4096), whose 528 tiles fill the
// chip un-split and where the fold launch is a second pass over Sigma for nothing.
static bool joint_use_splitk(int64_t M, int cus)
{
    static const int sw = (int)env_int("GPE_JOINT_SPLITK", -1);
    if (sw >= 0)
        return sw != 0;
    const int64_t nt = (M + 127) / 128;
    return nt * (nt + 1) / 2 < 2 * (int64_t)cus;
}

struct JointDraws {
    const double* mean_q;
    const double* Z;
    int S;
    double* F;
    int64_t* argmax;
    double* fmax;
};

// kta / cov (either may be null) and, dr != null, the draws.  Called with the handle's mutex held.
static int joint_impl(gpe_ctx* c, const double* Xq, int64_t M, double jitter, double* kta, double* cov, int64_t ldc, const JointDraws* dr)
{
    hipStream_t s = c->stream;
    digest_kernel(c);
    const int64_t N = c->N;
    const int P = c->P;
    PhaseDrain pd(c);
    const bool want_cov = cov != nullptr || dr != nullptr;
    gpe_ctx* sc = nullptr;
    if (want_cov) {
        const int e = joint_scratch(c, M, &sc);
        if (e)
            return e;
    }
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device);
    // the split's k range runs to N rounded up to the k step over zero columns of Zt
    const int64_t N16 = round_up(N, 16);
    const int64_t mc_max = round_up(M, 64);
    QtBufs b = served_layout(c, mc_max, N16); // (GPE_QUERY_T is not asked here)
    // the split reads Zt tile by tile, the points contiguous: with fewer samples than one outer panel (the N x M layout: Z by the
    // blocked solve, the samples contiguous) the composed covariance path only
    const bool splitk = b.transposed && joint_use_splitk(M, cus);
    const int nch = want_cov && splitk ? joint_cov_chunks(M, N, cus) : 0;
    const int ncols = dr ? dr->S * P : 0;
    const int64_t nt = (M + 127) / 128, nitems = nt * (nt + 1) / 2 * std::max(nch, 0);
    const size_t n_z = (size_t)M * ncols, n_mq = dr && dr->mean_q ? (size_t)M * P : 0, n_am = 2 * (size_t)ncols;
    double *dPartM = nullptr, *dZn = nullptr, *dF = nullptr, *dMq = nullptr, *dAm = nullptr;
    GemmItem* dItems = nullptr;
    int32_t* dBins = nullptr;
    QueryScratch qs(c);
    if (const int e = qs.carve([&](Carver& cv) {
            qt_carve(b, cv);
            dPartM = cv.take<double>((size_t)nch * (size_t)(b.ldq * M)); // the partial matrices, ldq x M each
            dItems = cv.take<GemmItem>((size_t)nitems);
            dBins = cv.take<int32_t>((size_t)nitems + 1);
            dZn = cv.take<double>(n_z);
            dF = cv.take<double>(n_z);
            dMq = cv.take<double>(n_mq);
            dAm = cv.take<double>(n_am);
        }))
        return e;

    // (profiling: the call's own phases — Z, Sigma, the factorisation, the draws — for gpe_joint_phase_ms)
    Marks mk(c->pool, s, c->prof);
    const int t0 = mk.mark();
    chunk_begin(c, b, want_cov);
    if (want_cov && b.n_zt > (size_t)(N * b.ldq)) // (the zero columns behind Zt's N)
        HIPCHK(c, hipMemsetAsync(b.dZt + N * b.ldq, 0, sizeof(double) * (b.n_zt - (size_t)(N * b.ldq)), s));
    chunk_head(c, b, Xq, true, M, true, kta != nullptr || dr != nullptr, kta, 0, M);
    ZView z;
    if (want_cov)
        z = chunk_solve(c, b, M); // gp.hpp:620
    const int t1 = mk.mark();
    std::vector<GemmItem> items; // (host copies of the launch list: alive until the stream has been waited for, below)
    std::vector<int32_t> bins;
    if (want_cov && splitk) {
        // one workgroup per (lower tile, k chunk), in the order of gpe_debug_cov_plan; then the fold
        std::vector<int64_t> rows((size_t)nitems * 5);
        (void)joint_cov_plan(M, N, cus, rows.data(), nitems);
        items.resize((size_t)nitems);
        bins.resize((size_t)nitems + 1);
        const int64_t pstride = b.ldq * M;
        for (int64_t q = 0; q < nitems; ++q) {
            const int64_t ti = rows[5 * q], tj = rows[5 * q + 1], k0 = rows[5 * q + 2], k1 = round_up(rows[5 * q + 3], 16), slot = rows[5 * q + 4];
            GemmItem& it = items[(size_t)q];
            memset(&it, 0, sizeof(it));
            it.A = b.dZt + ti * 128 + k0 * b.ldq;
            it.B = b.dZt + tj * 128 + k0 * b.ldq;
            it.C = dPartM + slot * pstride + ti * 128 + tj * 128 * b.ldq;
            it.k = (int32_t)(k1 - k0);
            const int mr = (int)std::min<int64_t>(128, M - ti * 128), nc = (int)std::min<int64_t>(128, M - tj * 128);
            it.flags = (mr << 8) | (nc << 16);
            it.nch = 1; // a chunk is a product of its own here: no arrival counters, the fold launch adds the partials up
            bins[(size_t)q] = (int32_t)q;
        }
        bins[(size_t)nitems] = (int32_t)nitems;
        HIPCHK(c, hipMemcpyAsync(dItems, items.data(), sizeof(GemmItem) * items.size(), hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(dBins, bins.data(), sizeof(int32_t) * bins.size(), hipMemcpyHostToDevice, s));
        PhaseScope ps(c, GPE_PH_QUERY, (double)M * M * N);
        launch_gemm_items(s, dItems, dBins, (int)nitems, b.ldq, 128, nullptr, 1, 0);
        launch_cov_fold(s, dPartM, b.ldq, pstride, nch, b.dQt, b.ldq, M, c->kp, jitter, sc->dKhost, sc->ld);
    }
    else if (want_cov) {
        // the composed path: the kernel matrix of V (+ jitter), the triangular matrix-core update with k = N, the mirror
        PhaseScope ps(c, GPE_PH_QUERY, (double)M * M * N);
        KParams kj = c->kp;
        kj.diag_add = jitter;
        (void)launch_build_K(s, b.dQt, b.ldq, M, kj, sc->dKhost, sc->ld);
        GemmArgs g{};
        g.C = sc->dKhost;
        g.ldc = sc->ld;
        z_operands(g, z, z);
        g.m = M;
        g.n = M;
        g.k = N;
        g.tri = 1;
        g.tile = b.qtile;
        launch_gemm_sub(s, g);
        launch_symmetrize_from_lower(s, sc->dKhost, sc->ld, M);
    }
    const int t2 = mk.mark();
    int t3 = -1, t4 = -1;
    if (cov)
        HIPCHK(c, copy2d_to_host(cov, ldc, sc->dKhost, sc->ld, M, M, s));
    if (dr && ncols > 0) {
        HIPCHK(c, hipMemcpyAsync(dZn, dr->Z, sizeof(double) * n_z, hipMemcpyHostToDevice, s));
        if (n_mq)
            HIPCHK(c, hipMemcpyAsync(dMq, dr->mean_q, sizeof(double) * n_mq, hipMemcpyHostToDevice, s));
    }
    if (const int e = stream_wait(c, "joint posterior", true))
        return e;
    int rc = GPE_OK;
    if (dr) {
        // C = chol(Sigma + jitter I) by the engine's factorisation schedule, in the scratch context (Sigma is complete: the
        // model's stream has been waited for)
        {
            DevGuard g(sc);
            const auto t0 = std::chrono::steady_clock::now();
            rc = compute_enqueue(sc);
            if (rc == GPE_OK)
                rc = compute_finish(sc);
            if (rc < 0)
                c->err = "joint posterior: factorisation: " + sc->err;
            c->joint_ms[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        if (rc == GPE_OK && ncols > 0) {
            t3 = mk.mark();
            {
                PhaseScope ps(c, GPE_PH_QUERY, (double)M * M * ncols);
                launch_draws(s, sc->dA, sc->ld, M, dZn, n_mq ? dMq : nullptr, b.dKta, b.mc_max, dr->S, ncols, dF);
                if (dr->argmax || dr->fmax)
                    launch_argmax(s, dF, M, ncols, dAm);
            }
            t4 = mk.mark();
            std::vector<double> am(n_am);
            if (dr->F)
                HIPCHK(c, hipMemcpyAsync(dr->F, dF, sizeof(double) * n_z, hipMemcpyDeviceToHost, s));
            if (dr->argmax || dr->fmax)
                HIPCHK(c, hipMemcpyAsync(am.data(), dAm, sizeof(double) * n_am, hipMemcpyDeviceToHost, s));
            rc = stream_wait(c, "joint posterior", true);
            if (rc == GPE_OK)
                for (int q = 0; q < ncols; ++q) {
                    if (dr->fmax)
                        dr->fmax[q] = am[2 * (size_t)q];
                    if (dr->argmax)
                        memcpy(dr->argmax + q, &am[2 * (size_t)q + 1], sizeof(int64_t));
                }
        }
    }
    if (c->prof) { // (every stream wait above has passed: the events are complete)
        c->joint_ms[0] = mk.ms(t0, t1);
        c->joint_ms[1] = mk.ms(t1, t2);
        c->joint_ms[3] = mk.ms(t3, t4);
        if (!dr)
            c->joint_ms[2] = 0.0;
    }
    return rc;
}

static int joint_check(gpe_ctx* c, const double* Xq, int64_t M, double jitter)
{
    if (!c || M < 0 || !(jitter >= 0.0) || !std::isfinite(jitter) || (M > 0 && !Xq))
        return GPE_ERR_ARG;
    if (!c->have_L)
        return GPE_ERR_STATE;
    if (c->host_K)
        return GPE_ERR_UNSUPPORTED;
    if (M > joint_max_points(c))
        return GPE_ERR_ARG;
    return GPE_OK;
}

int gpe_joint_query(gpe_handle c, const double* Xq, int64_t M, double jitter, double* kta, double* cov, int64_t ldc)
{
    const int e = joint_check(c, Xq, M, jitter);
    if (e)
        return e;
    if (cov && ldc < M)
        return GPE_ERR_ARG;
    if (M == 0 || (!kta && !cov))
        return GPE_OK;
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    return joint_impl(c, Xq, M, jitter, kta, cov, ldc, nullptr);
}

int gpe_joint_draws(gpe_handle c, const double* Xq, int64_t M, double jitter, const double* mean_q, const double* Z, int S, double* F,
                    int64_t* argmax, double* fmax)
{
    if (S < 0)
        return GPE_ERR_ARG;
    const int e = joint_check(c, Xq, M, jitter);
    if (e)
        return e;
    if (S > 0 && M > 0 && !Z)
        return GPE_ERR_ARG;
    if (M == 0)
        return GPE_OK;
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    const JointDraws dr{mean_q, Z, S, F, argmax, fmax};
    return joint_impl(c, Xq, M, jitter, nullptr, nullptr, 0, &dr);
}

int gpe_joint_max_points(gpe_handle c, int64_t* M_max)
{
    if (!c || !M_max)
        return GPE_ERR_ARG;
    if (c->N <= 0)
        return GPE_ERR_STATE;
    *M_max = joint_max_points(c);
    return GPE_OK;
}

int gpe_joint_phase_ms(gpe_handle c, double* ms4) { return phase_ms_get(c, &gpe_ctx::joint_ms, ms4); }

int gpe_debug_cov_plan(int64_t M, int64_t N, int cus, int64_t* out, int64_t cap_rows) { return joint_cov_plan(M, N, cus, out, cap_rows); }
