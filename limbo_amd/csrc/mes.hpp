// mes.hpp — max-value entropy search in the log domain (include/gpe_mes.h): host side.  Kernel: mes.hip.
// A part of engine.hip's translation unit (included there, once, behind cei.hpp, whose chunking it follows).
#pragma once

// what both entry points check before anything needs the device
static bool mes_args_ok(int J, int K, const double* ystar)
{
    if (J < 1 || J > GPE_MES_MAX_OUTPUTS || K < 1 || K > GPE_MES_MAX_SAMPLES || !ystar)
        return false;
    for (int i = 0; i < J * K; ++i)
        if (!std::isfinite(ystar[i]))
            return false;
    return true;
}

// The kernel alone, on host-supplied beliefs: any handle, computed or not (its device, stream and scratch are all it takes)
int gpe_mes_values(gpe_handle c, int J, int K, const double* ystar, const double* mu, const double* sd, int64_t M, double* logmes, double* terms,
                   double* partials)
{
    if (M < 0 || !mes_args_ok(J, K, ystar))
        return GPE_ERR_ARG;
    if (M == 0)
        return GPE_OK;
    if (!c || !logmes || !mu || !sd)
        return GPE_ERR_ARG;
    for (int64_t i = 0; i < M * J; ++i)
        if (sd[i] < 0.0)
            return GPE_ERR_ARG;
    if (c->host_K)
        return GPE_ERR_UNSUPPORTED;
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t s = c->stream;
    const int64_t mc_max = std::min<int64_t>(M, 16384); // candidates on the device at once
    double *dY = nullptr, *dMu = nullptr, *dSd = nullptr, *dV = nullptr, *dT = nullptr, *dP = nullptr;
    QueryScratch qs(c);
    if (const int e = qs.carve([&](Carver& cv) {
            dY = cv.take<double>((size_t)(J * K));
            dMu = cv.take<double>((size_t)(J * mc_max));
            dSd = cv.take<double>((size_t)(J * mc_max));
            dV = cv.take<double>((size_t)mc_max);
            dT = cv.take<double>((size_t)(J * mc_max));
            dP = cv.take<double>((size_t)(2 * J * mc_max));
        }))
        return e;
    HIPCHK(c, hipMemcpyAsync(dY, ystar, sizeof(double) * (size_t)(J * K), hipMemcpyHostToDevice, s));
    for (int64_t m0 = 0; m0 < M; m0 += mc_max) {
        const int64_t mc = std::min<int64_t>(mc_max, M - m0);
        HIPCHK(c, copy2d_from_host(dMu, mc_max, mu + m0, M, mc, J, s));
        HIPCHK(c, copy2d_from_host(dSd, mc_max, sd + m0, M, mc, J, s));
        MesArgs q{};
        q.J = J;
        q.K = K;
        for (int j = 0; j < J; ++j)
            q.col[j] = j;
        q.ystar = dY;
        q.mu = dMu;
        q.sd = dSd;
        q.ldmu = q.lds = mc_max;
        q.M = mc;
        q.logmes = dV;
        q.terms = terms ? dT : nullptr;
        q.partials = partials ? dP : nullptr;
        q.ldt = q.ldp = mc_max;
        launch_mes(s, q);
        HIPCHK(c, hipMemcpyAsync(logmes + m0, dV, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s));
        if (terms)
            HIPCHK(c, copy2d_to_host(terms + m0, M, dT, mc_max, mc, J, s));
        if (partials)
            HIPCHK(c, copy2d_to_host(partials + m0, M, dP, mc_max, mc, 2 * J, s));
        if (const int e = stream_wait(c, "mes_values", true))
            return e;
    }
    return GPE_OK;
}

// Called with the handle's mutex held; M > 0, arguments checked.
static int mes_impl(gpe_ctx* c, int J, const int* outs, int K, const double* ystar, const double* Xc, int64_t M, const double* mean_add,
                    double var_add, double* logmes, double* terms, double* partials, double* mu, double* var)
{
    hipStream_t s = c->stream;
    digest_kernel(c);
    const int64_t N = c->N;
    const int D = c->D;
    PhaseDrain pd(c);
    // the chunk of a query, as cei_impl's candidates (a candidate's answer must not depend on the batch around it)
    const int64_t mc_max = qt_serves(c) ? qt_rows_per_chunk(N, M) : std::min<int64_t>(nm_cols_per_chunk(c->ld, M), kKgNmChunk);
    QtBufs bc = served_layout(c, mc_max, N);
    double *dY = nullptr, *dAdd = nullptr, *dV = nullptr, *dT = nullptr, *dP = nullptr, *dMu = nullptr;
    QueryScratch qs(c);
    if (const int e = qs.carve([&](Carver& cv) {
            qt_carve(bc, cv);
            dY = cv.take<double>((size_t)(J * K));
            dAdd = cv.take<double>((size_t)(J * mc_max));
            dV = cv.take<double>((size_t)mc_max);
            dT = cv.take<double>((size_t)(J * mc_max));
            dP = cv.take<double>((size_t)(2 * J * mc_max));
            dMu = cv.take<double>((size_t)(J * mc_max));
        }))
        return e;
    HIPCHK(c, hipMemcpyAsync(dY, ystar, sizeof(double) * (size_t)(J * K), hipMemcpyHostToDevice, s));

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
            HIPCHK(c, copy2d_from_host(dAdd, mc_max, mean_add + m0, M, mc, J, s));
        const int u1 = mk.mark();
        {
            PhaseScope ps(c, GPE_PH_QUERY, 0.0);
            MesArgs q{};
            q.J = J;
            q.K = K;
            for (int j = 0; j < J; ++j)
                q.col[j] = outs[j];
            q.ystar = dY;
            q.mu = bc.dKta;
            q.ldmu = bc.mc_max;
            q.add = mean_add ? dAdd : nullptr;
            q.lda = mc_max;
            q.var = bc.dVar;
            q.var_add = var_add;
            q.M = mc;
            q.logmes = dV;
            q.terms = terms ? dT : nullptr;
            q.partials = partials ? dP : nullptr;
            q.mu_out = mu ? dMu : nullptr;
            q.ldt = q.ldp = q.ldm = mc_max;
            launch_mes(s, q);
        }
        const int u2 = mk.mark();
        if (logmes)
            HIPCHK(c, hipMemcpyAsync(logmes + m0, dV, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s));
        if (terms)
            HIPCHK(c, copy2d_to_host(terms + m0, M, dT, mc_max, mc, J, s));
        if (partials)
            HIPCHK(c, copy2d_to_host(partials + m0, M, dP, mc_max, mc, 2 * J, s));
        if (mu)
            HIPCHK(c, copy2d_to_host(mu + m0, M, dMu, mc_max, mc, J, s));
        if (var)
            HIPCHK(c, hipMemcpyAsync(var + m0, bc.dVar, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s));
        const int u3 = mk.mark();
        rc = stream_wait(c, "mes_batch", true);
        ms[0] += mk.ms(u0, u1);
        ms[1] += mk.ms(u1, u2);
        ms[2] += mk.ms(u2, u3);
    }
    if (c->prof && rc == GPE_OK)
        for (int q = 0; q < 3; ++q)
            c->mes_ms[q] = ms[q];
    return rc;
}

int gpe_mes_batch(gpe_handle c, int J, const int* outs, int K, const double* ystar, const double* Xc, int64_t M, const double* mean_add,
                  double var_add, double* logmes, double* terms, double* partials, double* mu, double* var)
{
    if (!c || M < 0 || !(var_add >= 0.0) || !std::isfinite(var_add) || (M > 0 && !Xc) || !outs || !mes_args_ok(J, K, ystar))
        return GPE_ERR_ARG;
    if (!c->have_L)
        return GPE_ERR_STATE;
    if (c->host_K)
        return GPE_ERR_UNSUPPORTED;
    for (int j = 0; j < J; ++j) {
        if (outs[j] < 0 || outs[j] >= c->P)
            return GPE_ERR_ARG;
        for (int i = 0; i < j; ++i)
            if (outs[i] == outs[j])
                return GPE_ERR_ARG;
    }
    if (M == 0 || (!logmes && !terms && !partials && !mu && !var))
        return GPE_OK;
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    return mes_impl(c, J, outs, K, ystar, Xc, M, mean_add, var_add, logmes, terms, partials, mu, var);
}

int gpe_mes_phase_ms(gpe_handle c, double* ms3)
{
    if (!c || !ms3)
        return GPE_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    for (int q = 0; q < 3; ++q)
        ms3[q] = c->mes_ms[q];
    return GPE_OK;
}
