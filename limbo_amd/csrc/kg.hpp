// kg.hpp — the knowledge gradient over a finite alternative set (include/gpe_kg.h): host side.  Kernel: kg.hip.
// A part of engine.hip's translation unit (included there, once, behind acq.hpp, whose chunk rule and chunk steps it shares).
#pragma once

// Called with the handle's mutex held; A in [1, GPE_KG_MAX_ALTERNATIVES], M > 0, arguments checked.
static int kg_impl(gpe_ctx* c, const double* Xa, int64_t A, const double* mu_a, const double* Xc, int64_t M, const double* mu_c,
                   double obs_noise, int with_self, double* kg, double* var_c, double* cov, int64_t ldc)
{
    hipStream_t s = c->stream;
    digest_kernel(c);
    const int64_t N = c->N;
    const int D = c->D;
    PhaseDrain pd(c);
    // two sets of chunk buffers in one lease of the scratch: the alternatives' (resident for the call: Z_a, a) and a candidate chunk's
    const int64_t ma_max = round_up(A, 64), mc_max = cand_chunk_max(c, M);
    QtBufs ba = served_layout(c, ma_max, N), bc = served_layout(c, mc_max, N);
    const int64_t ldx = ma_max + 16; // the cross-covariance: A x mc, column-major, alternatives contiguous (even: 16-byte columns)
    double *dA = nullptr, *dC = nullptr, *dKg = nullptr, *dMu = nullptr;
    QueryScratch qs(c);
    if (const int e = qs.carve([&](Carver& cv) {
            qt_carve(ba, cv);
            qt_carve(bc, cv);
            dA = cv.take<double>((size_t)ma_max);
            dC = cv.take<double>((size_t)(ldx * mc_max));
            dKg = cv.take<double>((size_t)mc_max);
            dMu = cv.take<double>((size_t)mc_max);
        }))
        return e;
    bc.dXp = ba.dXp; // (the panel inverses are the model's: one set serves both)

    Marks mk(c->pool, s, c->prof);
    double ms[4] = {0, 0, 0, 0};
    // the alternatives, once: Z_a = L^-1 k(X, Xa) and a
    const int t0 = mk.mark();
    chunk_begin(c, ba, true);
    chunk_head(c, ba, Xa, true, A, true, mu_a == nullptr, nullptr, 0, A);
    const ZView za = chunk_solve(c, ba, A);
    if (mu_a)
        HIPCHK(c, hipMemcpyAsync(dA, mu_a, sizeof(double) * (size_t)A, hipMemcpyHostToDevice, s));
    const double* da = mu_a ? dA : ba.dKta; // (output 0: the first column of kta)
    const int t1 = mk.mark();
    int rc = GPE_OK;
    for (int64_t m0 = 0; m0 < M && rc == GPE_OK; m0 += mc_max) {
        const int64_t mc = std::min<int64_t>(mc_max, M - m0);
        const bool want_kta = with_self && !mu_c;
        const int u0 = mk.mark();
        const ZView zc = cand_chunk(c, bc, Xc + m0 * D, mc, want_kta);
        cross_cov(c, ba, za, A, bc, zc, mc, dC, ldx);
        if (with_self && mu_c)
            HIPCHK(c, hipMemcpyAsync(dMu, mu_c + m0, sizeof(double) * (size_t)mc, hipMemcpyHostToDevice, s));
        const int u1 = mk.mark();
        if (kg) {
            PhaseScope ps(c, GPE_PH_QUERY, 0.0);
            launch_kg_envelope(s, da, (int)A, dC, ldx, mc, bc.dVar, obs_noise, with_self, mu_c ? dMu : bc.dKta, dKg, nullptr);
        }
        const int u2 = mk.mark();
        if (kg)
            HIPCHK(c, hipMemcpyAsync(kg + m0, dKg, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s));
        if (var_c)
            HIPCHK(c, hipMemcpyAsync(var_c + m0, bc.dVar, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s));
        if (cov)
            HIPCHK(c, copy2d_to_host(cov + m0 * ldc, ldc, dC, ldx, A, mc, s));
        const int u3 = mk.mark();
        rc = stream_wait(c, "kg_batch", true);
        ms[1] += mk.ms(u0, u1);
        ms[2] += mk.ms(u1, u2);
        ms[3] += mk.ms(u2, u3);
    }
    if (c->prof && rc == GPE_OK) {
        ms[0] = mk.ms(t0, t1);
        for (int q = 0; q < 4; ++q)
            c->kg_ms[q] = ms[q];
    }
    return rc;
}

int gpe_kg_batch(gpe_handle c, const double* Xa, int64_t A, const double* mu_a, const double* Xc, int64_t M, const double* mu_c,
                 double obs_noise, int with_self, double* kg, double* var_c, double* cov, int64_t ldc)
{
    if (!c || A < 1 || A > GPE_KG_MAX_ALTERNATIVES || M < 0 || !(obs_noise >= 0.0) || !std::isfinite(obs_noise) || !Xa || (M > 0 && !Xc)
        || (cov && ldc < A))
        return GPE_ERR_ARG;
    if (!c->have_L)
        return GPE_ERR_STATE;
    if (c->host_K)
        return GPE_ERR_UNSUPPORTED;
    if (M == 0 || (!kg && !var_c && !cov))
        return GPE_OK;
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    return kg_impl(c, Xa, A, mu_a, Xc, M, mu_c, obs_noise, with_self ? 1 : 0, kg, var_c, cov, ldc);
}

// The envelope alone, on host-supplied beliefs: any handle, computed or not (its device, stream and scratch are all it takes)
int gpe_kg_envelope(gpe_handle c, const double* a, int64_t A, const double* B, int64_t ldb, int64_t M, double* kg, int32_t* nseg)
{
    if (!c || A < 1 || A > GPE_KG_MAX_ALTERNATIVES || M < 0 || ldb < A || !a || (M > 0 && (!B || !kg)))
        return GPE_ERR_ARG;
    if (c->host_K)
        return GPE_ERR_UNSUPPORTED;
    if (M == 0)
        return GPE_OK;
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t s = c->stream;
    const int64_t mc_max = std::min<int64_t>(M, kValuesChunk); // columns on the device at once
    double *dA = nullptr, *dB = nullptr, *dKg = nullptr;
    int* dSeg = nullptr;
    QueryScratch qs(c);
    if (const int e = qs.carve([&](Carver& cv) {
            dA = cv.take<double>((size_t)A);
            dB = cv.take<double>((size_t)(A * mc_max));
            dKg = cv.take<double>((size_t)mc_max);
            dSeg = cv.take<int>((size_t)mc_max);
        }))
        return e;
    HIPCHK(c, hipMemcpyAsync(dA, a, sizeof(double) * (size_t)A, hipMemcpyHostToDevice, s));
    for (int64_t m0 = 0; m0 < M; m0 += mc_max) {
        const int64_t mc = std::min<int64_t>(mc_max, M - m0);
        HIPCHK(c, copy2d_from_host(dB, A, B + m0 * ldb, ldb, A, mc, s));
        launch_kg_envelope(s, dA, (int)A, dB, A, mc, nullptr, 0.0, 0, nullptr, dKg, dSeg);
        HIPCHK(c, hipMemcpyAsync(kg + m0, dKg, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s));
        if (nseg)
            HIPCHK(c, hipMemcpyAsync(nseg + m0, dSeg, sizeof(int) * (size_t)mc, hipMemcpyDeviceToHost, s));
        if (const int e = stream_wait(c, "kg_envelope", true))
            return e;
    }
    return GPE_OK;
}

int gpe_kg_phase_ms(gpe_handle c, double* ms4) { return phase_ms_get(c, &gpe_ctx::kg_ms, ms4); }
