// nei.hpp — noisy expected improvement in the log domain (include/gpe_nei.h): host side.  Kernels: nei.hip.
// A part of engine.hip's translation unit (included there, once, behind joint.hpp and acq.hpp, whose helpers it shares).
#pragma once

// Candidates on the device at once: U (B x chunk) and cmean (S x chunk) lie beside the chunk's own buffers
static const int64_t kNeiChunk = kValuesChunk;
// The tile of the solve by L_b and of the product Z^T U: B <= 1024 rows never fill the chip with 128 x 128 tiles, and a tile picked
// by the size of each product would come from the chunk — a candidate's answer must not depend on the batch around it
static const int kNeiTile = 64;

extern "C++" {
namespace {
// two events of the handle's pool for the length of a call, returned on every way out of it
struct NeiEvents {
    std::vector<hipEvent_t>& pool;
    hipEvent_t e0, e1;
    explicit NeiEvents(std::vector<hipEvent_t>& pool_) : pool(pool_), e0(get_event(pool_)), e1(get_event(pool_)) {}
    NeiEvents(const NeiEvents&) = delete;
    ~NeiEvents()
    {
        pool.push_back(e0);
        pool.push_back(e1);
    }
};
} // namespace
} // extern "C++"

// what both entry points check before anything needs the device
static bool nei_samples_ok(int S, double xi)
{
    return S >= 1 && S <= GPE_NEI_MAX_SAMPLES && std::isfinite(xi);
}

// The kernel alone, on host-supplied conditional beliefs: any handle, computed or not (its device, stream and scratch are all it takes)
int gpe_lognei_values(gpe_handle c, int S, const double* fplus, double xi, const double* cmean, int64_t ldm, const double* csd, int64_t M,
                      double* lognei, double* terms)
{
    if (M < 0 || !nei_samples_ok(S, xi) || !fplus || ldm < S)
        return GPE_ERR_ARG;
    for (int i = 0; i < S; ++i)
        if (!std::isfinite(fplus[i]))
            return GPE_ERR_ARG;
    if (M == 0)
        return GPE_OK;
    if (!c || !lognei || !cmean || !csd)
        return GPE_ERR_ARG;
    for (int64_t i = 0; i < M; ++i)
        if (csd[i] < 0.0)
            return GPE_ERR_ARG;
    if (c->host_K)
        return GPE_ERR_UNSUPPORTED;
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t s = c->stream;
    const int64_t mc_max = std::min<int64_t>(M, kNeiChunk); // candidates on the device at once
    double *dFp = nullptr, *dCm = nullptr, *dSd = nullptr, *dV = nullptr, *dT = nullptr;
    QueryScratch qs(c);
    if (const int e = qs.carve([&](Carver& cv) {
            dFp = cv.take<double>((size_t)S);
            dCm = cv.take<double>((size_t)(S * mc_max));
            dSd = cv.take<double>((size_t)mc_max);
            dV = cv.take<double>((size_t)mc_max);
            dT = cv.take<double>(terms ? (size_t)(S * mc_max) : 0);
        }))
        return e;
    HIPCHK(c, hipMemcpyAsync(dFp, fplus, sizeof(double) * (size_t)S, hipMemcpyHostToDevice, s));
    for (int64_t m0 = 0; m0 < M; m0 += mc_max) {
        const int64_t mc = std::min<int64_t>(mc_max, M - m0);
        HIPCHK(c, copy2d_from_host(dCm, S, cmean + m0 * ldm, ldm, S, mc, s)); // (the first S rows of a column: nothing behind them)
        HIPCHK(c, hipMemcpyAsync(dSd, csd + m0, sizeof(double) * (size_t)mc, hipMemcpyHostToDevice, s));
        NeiArgs q{};
        q.S = S;
        q.fplus = dFp;
        q.xi = xi;
        q.cmean = dCm;
        q.ldm = S;
        q.csd = dSd;
        q.M = mc;
        q.lognei = dV;
        q.terms = terms ? dT : nullptr;
        q.ldt = S;
        launch_lognei(s, q);
        HIPCHK(c, hipMemcpyAsync(lognei + m0, dV, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s));
        if (terms)
            HIPCHK(c, hipMemcpyAsync(terms + m0 * S, dT, sizeof(double) * (size_t)(S * mc), hipMemcpyDeviceToHost, s));
        if (const int e = stream_wait(c, "lognei_values", true))
            return e;
    }
    return GPE_OK;
}

// Called with the handle's mutex held; B in [1, GPE_NEI_MAX_BASELINE], M > 0, arguments checked.
static int nei_impl(gpe_ctx* c, int out, const double* Xb, int64_t B, const double* mean_b, double jitter, const double* Z, int S, double xi,
                    const double* Xc, int64_t M, const double* mean_add, double* lognei, double* fplus, double* mu, double* var, double* cvar,
                    double* cmean, int64_t ldm)
{
    hipStream_t s = c->stream;
    digest_kernel(c);
    const int64_t N = c->N;
    const int D = c->D;
    PhaseDrain pd(c);
    // Sigma_b is factored where the joint posterior's covariance is: the private scratch context, a full engine context whose factor
    // is then L_b and whose blocked solve serves the conditioning.  Every joint call shapes and fills that context anew.
    gpe_ctx* sc = nullptr;
    if (const int e = joint_scratch(c, B, &sc))
        return e;
    // two sets of chunk buffers in one lease of the scratch: the baseline's (resident for the call: Zt_b, mu_b) and a candidate chunk's
    const int64_t mb_max = round_up(B, 64), mc_max = cand_chunk_max(c, M, kNeiChunk);
    QtBufs bb = served_layout(c, mb_max, N), bc = served_layout(c, mc_max, N);
    const int64_t ldu = mb_max + 16; // c, then u in its place: B x mc, column-major, the baseline contiguous
    const int64_t ldcm = round_up(S, 16);
    double *dZn = nullptr, *dF = nullptr, *dMb = nullptr, *dFp = nullptr, *dU = nullptr, *dCm = nullptr, *dAdd = nullptr, *dMu = nullptr,
           *dCv = nullptr, *dV = nullptr;
    QueryScratch qs(c);
    if (const int e = qs.carve([&](Carver& cv) {
            qt_carve(bb, cv);
            qt_carve(bc, cv);
            dZn = cv.take<double>((size_t)(B * S));
            dF = cv.take<double>((size_t)(B * S));
            dMb = cv.take<double>((size_t)mb_max);
            dFp = cv.take<double>((size_t)ldcm);
            dU = cv.take<double>((size_t)(ldu * mc_max));
            dCm = cv.take<double>((size_t)(ldcm * mc_max));
            dAdd = cv.take<double>((size_t)mc_max);
            dMu = cv.take<double>((size_t)mc_max);
            dCv = cv.take<double>((size_t)mc_max);
            dV = cv.take<double>((size_t)mc_max);
        }))
        return e;
    bc.dXp = bb.dXp; // (the panel inverses are the model's: one set serves both)

    Marks mk(c->pool, s, c->prof);
    double ms[5] = {0, 0, 0, 0, 0};
    // ---- the baseline, once: Zt_b = (L^-1 k(X, Xb))^T, mu_b, Sigma_b by joint_impl's composed path
    const int t0 = mk.mark();
    chunk_begin(c, bb, true);
    chunk_head(c, bb, Xb, true, B, true, true, nullptr, 0, B);
    const ZView zb = chunk_solve(c, bb, B);
    {
        PhaseScope ps(c, GPE_PH_QUERY, (double)B * B * N);
        KParams kj = c->kp;
        kj.diag_add = jitter;
        (void)launch_build_K(s, bb.dQt, bb.ldq, B, kj, sc->dKhost, sc->ld);
        GemmArgs g{};
        g.C = sc->dKhost;
        g.ldc = sc->ld;
        z_operands(g, zb, zb);
        g.m = B;
        g.n = B;
        g.k = N;
        g.tri = 1;
        g.tile = bb.qtile;
        launch_gemm_sub(s, g);
        launch_symmetrize_from_lower(s, sc->dKhost, sc->ld, B);
    }
    HIPCHK(c, hipMemcpyAsync(dZn, Z, sizeof(double) * (size_t)(B * S), hipMemcpyHostToDevice, s));
    if (mean_b)
        HIPCHK(c, hipMemcpyAsync(dMb, mean_b, sizeof(double) * (size_t)B, hipMemcpyHostToDevice, s));
    const int t1 = mk.mark();
    if (const int e = stream_wait(c, "lognei_batch", true))
        return e;
    // ---- L_b = chol(Sigma_b) by the engine's factorisation schedule, in the scratch context (Sigma_b is complete: the model's stream
    // has been waited for); then the draws and their maxima
    int rc = GPE_OK;
    const auto h0 = std::chrono::steady_clock::now();
    {
        DevGuard g(sc);
        rc = compute_enqueue(sc);
        if (rc == GPE_OK)
            rc = compute_finish(sc);
        if (rc < 0)
            c->err = "noisy expected improvement: factorisation: " + sc->err;
    }
    const double fact_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count();
    if (rc != GPE_OK)
        return rc;
    const int t2 = mk.mark();
    {
        PhaseScope ps(c, GPE_PH_QUERY, (double)B * B * S);
        launch_draws(s, sc->dA, sc->ld, B, dZn, mean_b ? dMb : nullptr, bb.dKta + (int64_t)out * bb.mc_max, bb.mc_max, S, S, dF);
        launch_nei_colmax(s, dF, B, S, dFp);
    }
    if (fplus)
        HIPCHK(c, hipMemcpyAsync(fplus, dFp, sizeof(double) * (size_t)S, hipMemcpyDeviceToHost, s));
    const int t3 = mk.mark();

    // the solve by L_b launches on its context's stream: ordered against the model's by events, chunk by chunk
    NeiEvents ev(c->pool);
    for (int64_t m0 = 0; m0 < M && rc == GPE_OK; m0 += mc_max) {
        const int64_t mc = std::min<int64_t>(mc_max, M - m0);
        const int u0 = mk.mark();
        const ZView zc = cand_chunk(c, bc, Xc + m0 * D, mc, true);
        cross_cov(c, bb, zb, B, bc, zc, mc, dU, ldu); // c = k(Xb, Xc) - Zt_b Zt_c^T
        if (mean_add)
            HIPCHK(c, hipMemcpyAsync(dAdd, mean_add + m0, sizeof(double) * (size_t)mc, hipMemcpyHostToDevice, s));
        const int u1 = mk.mark();
        {
            // u = L_b^-1 c in place (the scratch context's blocked solve, tile fixed); cvar = var - |u|^2 and mu; cmean = mu + Z^T u
            PhaseScope ps(c, GPE_PH_QUERY, (double)B * B * mc + 2.0 * (double)B * S * mc);
            hipEventRecord(ev.e0, s);
            hipStreamWaitEvent(sc->stream, ev.e0, 0);
            trsm_left_blocked(sc, sc->dA, dU, ldu, B, mc, false, GPE_PH_QUERY, kNeiTile);
            hipEventRecord(ev.e1, sc->stream);
            hipStreamWaitEvent(s, ev.e1, 0);
            launch_nei_cond(s, dU, ldu, B, bc.dKta + (int64_t)out * bc.mc_max, mean_add ? dAdd : nullptr, bc.dVar, mc, S, dMu, dCv, dCm, ldcm);
            GemmArgs g{};
            g.C = dCm;
            g.ldc = ldcm;
            g.A = dZn; // opA(s, i) = Z[i + s B]
            g.lda = B;
            g.a_kmajor = 1;
            g.B = dU; // opB(m, i) = u[i + m ldu]
            g.ldb = ldu;
            g.b_kmajor = 1;
            g.m = S;
            g.n = mc;
            g.k = B;
            g.overwrite = 2;
            g.tile = kNeiTile;
            launch_gemm_sub(s, g);
        }
        const int u2 = mk.mark();
        if (lognei) {
            PhaseScope ps(c, GPE_PH_QUERY, 0.0);
            NeiArgs q{};
            q.S = S;
            q.fplus = dFp;
            q.xi = xi;
            q.cmean = dCm;
            q.ldm = ldcm;
            q.cvar = dCv;
            q.M = mc;
            q.lognei = dV;
            launch_lognei(s, q);
            HIPCHK(c, hipMemcpyAsync(lognei + m0, dV, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s));
        }
        if (mu)
            HIPCHK(c, hipMemcpyAsync(mu + m0, dMu, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s));
        if (var)
            HIPCHK(c, hipMemcpyAsync(var + m0, bc.dVar, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s));
        if (cvar)
            HIPCHK(c, hipMemcpyAsync(cvar + m0, dCv, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s));
        if (cmean)
            HIPCHK(c, copy2d_to_host(cmean + m0 * ldm, ldm, dCm, ldcm, S, mc, s));
        const int u3 = mk.mark();
        rc = stream_wait(c, "lognei_batch", true);
        ms[2] += mk.ms(u0, u1);
        ms[3] += mk.ms(u1, u2);
        ms[4] += mk.ms(u2, u3);
    }
    if (c->prof && rc == GPE_OK) {
        ms[0] = mk.ms(t0, t1);
        ms[1] = fact_ms + mk.ms(t2, t3);
        for (int q = 0; q < 5; ++q)
            c->nei_ms[q] = ms[q];
    }
    return rc;
}

int gpe_lognei_batch(gpe_handle c, int out, const double* Xb, int64_t B, const double* mean_b, double jitter, const double* Z, int S, double xi,
                     const double* Xc, int64_t M, const double* mean_add, double* lognei, double* fplus, double* mu, double* var, double* cvar,
                     double* cmean, int64_t ldm)
{
    if (!c || B < 1 || B > GPE_NEI_MAX_BASELINE || !nei_samples_ok(S, xi) || M < 0 || !(jitter >= 0.0) || !std::isfinite(jitter) || !Xb || !Z
        || (M > 0 && !Xc) || (cmean && ldm < S))
        return GPE_ERR_ARG;
    for (int64_t i = 0; i < B * S; ++i)
        if (!std::isfinite(Z[i]))
            return GPE_ERR_ARG;
    if (!c->have_L)
        return GPE_ERR_STATE;
    if (c->host_K)
        return GPE_ERR_UNSUPPORTED;
    if (out < 0 || out >= c->P || B > joint_max_points(c)) // (the baseline is resident like a joint call's points: one chunk of the model's)
        return GPE_ERR_ARG;
    if (M == 0 || (!lognei && !fplus && !mu && !var && !cvar && !cmean))
        return GPE_OK;
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    return nei_impl(c, out, Xb, B, mean_b, jitter, Z, S, xi, Xc, M, mean_add, lognei, fplus, mu, var, cvar, cmean, ldm);
}

int gpe_nei_phase_ms(gpe_handle c, double* ms5) { return phase_ms_get(c, &gpe_ctx::nei_ms, ms5); }
