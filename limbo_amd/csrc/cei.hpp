// cei.hpp — constrained expected improvement in the log domain (include/gpe_cei.h): host side.  Kernel: cei.hip.
// A part of engine.hip's translation unit (included there, once, behind ehvi.hpp, whose chunking it follows).
#pragma once

// what both entry points check before anything needs the device
static bool cei_args_ok(int with_ei, double f_best, double xi, int C, const double* thr)
{
    if (C < 0 || C > GPE_CEI_MAX_CONSTRAINTS || (C > 0 && !thr))
        return false;
    for (int k = 0; k < C; ++k)
        if (!std::isfinite(thr[k]))
            return false;
    return !with_ei || (std::isfinite(f_best) && std::isfinite(xi));
}
static void cei_fill(CeiArgs& q, int with_ei, double f_best, double xi, int C, const double* thr)
{
    q.with_ei = with_ei ? 1 : 0;
    q.C = C;
    q.f_best = with_ei ? f_best : 0.0;
    q.xi = with_ei ? xi : 0.0;
    for (int k = 0; k < C; ++k)
        q.thr[k] = thr[k];
}

// The kernel alone, on host-supplied beliefs: any handle, computed or not (its device, stream and scratch are all it takes)
int gpe_logcei_values(gpe_handle c, int with_ei, double f_best, double xi, int C, const double* thr, const double* mu0, const double* s0,
                      const double* mu_c, const double* s_c, int64_t M, double* logcei, double* terms, double* partials)
{
    if (M < 0 || !cei_args_ok(with_ei, f_best, xi, C, thr))
        return GPE_ERR_ARG;
    if (M == 0)
        return GPE_OK;
    if (!c || !logcei || (with_ei && (!mu0 || !s0)) || (C > 0 && (!mu_c || !s_c)))
        return GPE_ERR_ARG;
    for (int64_t m = 0; m < M; ++m)
        if (with_ei && s0[m] < 0.0)
            return GPE_ERR_ARG;
    for (int64_t i = 0; i < M * C; ++i)
        if (s_c[i] < 0.0)
            return GPE_ERR_ARG;
    if (c->host_K)
        return GPE_ERR_UNSUPPORTED;
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t s = c->stream;
    const int64_t mc_max = std::min<int64_t>(M, 16384); // candidates on the device at once
    const int B = 1 + C;
    double *dMu = nullptr, *dSd = nullptr, *dV = nullptr, *dT = nullptr, *dP = nullptr;
    QueryScratch qs(c);
    if (const int e = qs.carve([&](Carver& cv) {
            dMu = cv.take<double>((size_t)(B * mc_max));
            dSd = cv.take<double>((size_t)(B * mc_max));
            dV = cv.take<double>((size_t)mc_max);
            dT = cv.take<double>((size_t)(B * mc_max));
            dP = cv.take<double>((size_t)(2 * B * mc_max));
        }))
        return e;
    for (int64_t m0 = 0; m0 < M; m0 += mc_max) {
        const int64_t mc = std::min<int64_t>(mc_max, M - m0);
        if (with_ei) {
            HIPCHK(c, hipMemcpyAsync(dMu, mu0 + m0, sizeof(double) * (size_t)mc, hipMemcpyHostToDevice, s));
            HIPCHK(c, hipMemcpyAsync(dSd, s0 + m0, sizeof(double) * (size_t)mc, hipMemcpyHostToDevice, s));
        }
        if (C > 0) {
            HIPCHK(c, copy2d_from_host(dMu + mc_max, mc_max, mu_c + m0, M, mc, C, s));
            HIPCHK(c, copy2d_from_host(dSd + mc_max, mc_max, s_c + m0, M, mc, C, s));
        }
        CeiArgs q{};
        cei_fill(q, with_ei, f_best, xi, C, thr);
        for (int j = 0; j < B; ++j)
            q.col[j] = j;
        q.mu = dMu;
        q.sd = dSd;
        q.ldmu = q.lds = mc_max;
        q.M = mc;
        q.logcei = dV;
        q.terms = terms ? dT : nullptr;
        q.partials = partials ? dP : nullptr;
        q.ldt = q.ldp = mc_max;
        launch_logcei(s, q);
        HIPCHK(c, hipMemcpyAsync(logcei + m0, dV, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s));
        if (terms)
            HIPCHK(c, copy2d_to_host(terms + m0, M, dT, mc_max, mc, B, s));
        if (partials)
            HIPCHK(c, copy2d_to_host(partials + m0, M, dP, mc_max, mc, 2 * B, s));
        if (const int e = stream_wait(c, "logcei_values", true))
            return e;
    }
    return GPE_OK;
}

// Called with the handle's mutex held; M > 0, arguments checked.
static int cei_impl(gpe_ctx* c, int with_ei, int out0, double f_best, double xi, int C, const int* con_outs, const double* thr, const double* Xc,
                    int64_t M, const double* mean_add, double var_add, double* logcei, double* terms, double* partials, double* mu, double* var)
{
    hipStream_t s = c->stream;
    digest_kernel(c);
    const int64_t N = c->N;
    const int D = c->D;
    const int B = 1 + C;
    PhaseDrain pd(c);
    // the chunk of a query, as ehvi_impl's candidates (a candidate's answer must not depend on the batch around it)
    const int64_t mc_max = qt_serves(c) ? qt_rows_per_chunk(N, M) : std::min<int64_t>(nm_cols_per_chunk(c->ld, M), kKgNmChunk);
    QtBufs bc = served_layout(c, mc_max, N);
    double *dAdd = nullptr, *dV = nullptr, *dT = nullptr, *dP = nullptr, *dMu = nullptr;
    QueryScratch qs(c);
    if (const int e = qs.carve([&](Carver& cv) {
            qt_carve(bc, cv);
            dAdd = cv.take<double>((size_t)(B * mc_max));
            dV = cv.take<double>((size_t)mc_max);
            dT = cv.take<double>((size_t)(B * mc_max));
            dP = cv.take<double>((size_t)(2 * B * mc_max));
            dMu = cv.take<double>((size_t)(B * mc_max));
        }))
        return e;

    Marks mk(c->pool, s, c->prof);
    double ms[3] = {0, 0, 0};
    chunk_begin(c, bc, true);
    int rc = GPE_OK;
    for (int64_t m0 = 0; m0 < M && rc == GPE_OK; m0 += mc_max) {
        const int64_t mc = std::min<int64_t>(mc_max, M - m0);
        const int u0 = mk.mark();
        // the chunk's head (with k^T alpha of every output), solve and variance as a query's
        chunk_head(c, bc, Xc + m0 * D, true, mc, true, true, nullptr, 0, mc);
        const ZView zc = chunk_solve(c, bc, mc);
        chunk_var(c, bc, mc, zc);
        if (mean_add)
            HIPCHK(c, copy2d_from_host(dAdd, mc_max, mean_add + m0, M, mc, B, s));
        const int u1 = mk.mark();
        {
            PhaseScope ps(c, GPE_PH_QUERY, 0.0);
            CeiArgs q{};
            cei_fill(q, with_ei, f_best, xi, C, thr);
            q.col[0] = out0;
            for (int k = 0; k < C; ++k)
                q.col[1 + k] = con_outs[k];
            q.mu = bc.dKta;
            q.ldmu = bc.mc_max;
            q.add = mean_add ? dAdd : nullptr;
            q.lda = mc_max;
            q.var = bc.dVar;
            q.var_add = var_add;
            q.M = mc;
            q.logcei = dV;
            q.terms = terms ? dT : nullptr;
            q.partials = partials ? dP : nullptr;
            q.mu_out = mu ? dMu : nullptr;
            q.ldt = q.ldp = q.ldm = mc_max;
            launch_logcei(s, q);
        }
        const int u2 = mk.mark();
        if (logcei)
            HIPCHK(c, hipMemcpyAsync(logcei + m0, dV, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s));
        if (terms)
            HIPCHK(c, copy2d_to_host(terms + m0, M, dT, mc_max, mc, B, s));
        if (partials)
            HIPCHK(c, copy2d_to_host(partials + m0, M, dP, mc_max, mc, 2 * B, s));
        if (mu)
            HIPCHK(c, copy2d_to_host(mu + m0, M, dMu, mc_max, mc, B, s));
        if (var)
            HIPCHK(c, hipMemcpyAsync(var + m0, bc.dVar, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s));
        const int u3 = mk.mark();
        rc = stream_wait(c, "logcei_batch", true);
        ms[0] += mk.ms(u0, u1);
        ms[1] += mk.ms(u1, u2);
        ms[2] += mk.ms(u2, u3);
    }
    if (c->prof && rc == GPE_OK)
        for (int q = 0; q < 3; ++q)
            c->cei_ms[q] = ms[q];
    return rc;
}

int gpe_logcei_batch(gpe_handle c, int with_ei, int out0, double f_best, double xi, int C, const int* con_outs, const double* thr, const double* Xc,
                     int64_t M, const double* mean_add, double var_add, double* logcei, double* terms, double* partials, double* mu, double* var)
{
    if (!c || M < 0 || !(var_add >= 0.0) || !std::isfinite(var_add) || (M > 0 && !Xc) || !cei_args_ok(with_ei, f_best, xi, C, thr)
        || (C > 0 && !con_outs))
        return GPE_ERR_ARG;
    if (!c->have_L)
        return GPE_ERR_STATE;
    if (c->host_K)
        return GPE_ERR_UNSUPPORTED;
    if (out0 < 0 || out0 >= c->P)
        return GPE_ERR_ARG;
    for (int k = 0; k < C; ++k) {
        if (con_outs[k] < 0 || con_outs[k] >= c->P || con_outs[k] == out0)
            return GPE_ERR_ARG;
        for (int j = 0; j < k; ++j)
            if (con_outs[j] == con_outs[k])
                return GPE_ERR_ARG;
    }
    if (M == 0 || (!logcei && !terms && !partials && !mu && !var))
        return GPE_OK;
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    return cei_impl(c, with_ei, out0, f_best, xi, C, con_outs, thr, Xc, M, mean_add, var_add, logcei, terms, partials, mu, var);
}

int gpe_cei_phase_ms(gpe_handle c, double* ms3)
{
    if (!c || !ms3)
        return GPE_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    for (int q = 0; q < 3; ++q)
        ms3[q] = c->cei_ms[q];
    return GPE_OK;
}
