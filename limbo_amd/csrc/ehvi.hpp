// ehvi.hpp — the two-objective expected hypervolume improvement over a Pareto front (include/gpe_ehvi.h): host side.  Kernel: ehvi.hip.
// A part of engine.hip's translation unit (included there, once, behind kg.hpp, whose chunk size and helpers it shares).
#pragma once

// The prepared front: finite, strictly ascending in f1, strictly descending in f2, every point above ref in both.  O(n).
static bool ehvi_front_ok(const double* front, int64_t n, const double* ref)
{
    if (n < 0 || !ref || !std::isfinite(ref[0]) || !std::isfinite(ref[1]) || (n > 0 && !front))
        return false;
    for (int64_t i = 0; i < n; ++i) {
        const double f1 = front[2 * i], f2 = front[2 * i + 1];
        if (!std::isfinite(f1) || !std::isfinite(f2) || !(f1 > ref[0]) || !(f2 > ref[1]))
            return false;
        if (i > 0 && (!(f1 > front[2 * i - 2]) || !(f2 < front[2 * i - 1])))
            return false;
    }
    return true;
}

int gpe_ehvi2_front(const double* F, int64_t n, const double* ref, double* out, int64_t* n_out)
{
    if (n < 0 || !ref || !n_out || (n > 0 && (!F || !out)) || !std::isfinite(ref[0]) || !std::isfinite(ref[1]))
        return GPE_ERR_ARG;
    std::vector<std::pair<double, double>> p;
    p.reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const double f1 = F[2 * i], f2 = F[2 * i + 1];
        if (f1 != f1 || f2 != f2)
            return GPE_ERR_ARG;
        if (std::isfinite(f1) && std::isfinite(f2) && f1 > ref[0] && f2 > ref[1])
            p.emplace_back(f1, f2);
    }
    // ascending in (f1, f2); from the right a point stays when it is higher than everything to its right — of points equal in f1
    // the highest comes first, of duplicates one
    std::sort(p.begin(), p.end());
    std::vector<std::pair<double, double>> keep;
    double top = ref[1];
    for (size_t i = p.size(); i-- > 0;)
        if (p[i].second > top) {
            top = p[i].second;
            keep.push_back(p[i]);
        }
    const int64_t k = (int64_t)keep.size();
    for (int64_t i = 0; i < k; ++i) {
        out[2 * i] = keep[(size_t)(k - 1 - i)].first;
        out[2 * i + 1] = keep[(size_t)(k - 1 - i)].second;
    }
    *n_out = k;
    return GPE_OK;
}

// The strip sums alone, on host-supplied beliefs: any handle, computed or not (its device, stream and scratch are all it takes)
int gpe_ehvi2_values(gpe_handle c, const double* front, int64_t n, const double* ref, const double* mu1, const double* s1, const double* mu2,
                     const double* s2, int64_t M, double* ehvi, double* partials)
{
    if (M < 0 || n > GPE_EHVI_MAX_FRONT || !ehvi_front_ok(front, n, ref))
        return GPE_ERR_ARG;
    if (M == 0)
        return GPE_OK;
    if (!c || !mu1 || !s1 || !mu2 || !s2 || !ehvi)
        return GPE_ERR_ARG;
    for (int64_t m = 0; m < M; ++m)
        if (s1[m] < 0.0 || s2[m] < 0.0)
            return GPE_ERR_ARG;
    if (c->host_K)
        return GPE_ERR_UNSUPPORTED;
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t s = c->stream;
    const int64_t mc_max = std::min<int64_t>(M, 16384); // candidates on the device at once
    double *dF = nullptr, *dB = nullptr, *dE = nullptr, *dP = nullptr;
    QueryScratch qs(c);
    if (const int e = qs.carve([&](Carver& cv) {
            dF = cv.take<double>((size_t)(2 * std::max<int64_t>(n, 1)));
            dB = cv.take<double>((size_t)(4 * mc_max));
            dE = cv.take<double>((size_t)mc_max);
            dP = cv.take<double>((size_t)(4 * mc_max));
        }))
        return e;
    if (n > 0)
        HIPCHK(c, hipMemcpyAsync(dF, front, sizeof(double) * (size_t)(2 * n), hipMemcpyHostToDevice, s));
    const double* in[4] = {mu1, s1, mu2, s2};
    for (int64_t m0 = 0; m0 < M; m0 += mc_max) {
        const int64_t mc = std::min<int64_t>(mc_max, M - m0);
        for (int k = 0; k < 4; ++k)
            HIPCHK(c, hipMemcpyAsync(dB + k * mc_max, in[k] + m0, sizeof(double) * (size_t)mc, hipMemcpyHostToDevice, s));
        EhviArgs q{};
        q.front = dF;
        q.n = (int)n;
        q.r1 = ref[0];
        q.r2 = ref[1];
        q.mu1 = dB;
        q.s1 = dB + mc_max;
        q.mu2 = dB + 2 * mc_max;
        q.s2 = dB + 3 * mc_max;
        q.M = mc;
        q.ehvi = dE;
        q.partials = partials ? dP : nullptr;
        q.ldp = mc_max;
        launch_ehvi2(s, q);
        HIPCHK(c, hipMemcpyAsync(ehvi + m0, dE, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s));
        if (partials)
            HIPCHK(c, copy2d_to_host(partials + m0, M, dP, mc_max, mc, 4, s));
        if (const int e = stream_wait(c, "ehvi2_values", true))
            return e;
    }
    return GPE_OK;
}

// Called with the handle's mutex held; M > 0, arguments checked.
static int ehvi_impl(gpe_ctx* c, int out1, int out2, const double* Xc, int64_t M, const double* mean_add, double var_add, const double* front,
                     int64_t n, const double* ref, double* ehvi, double* partials, double* mu, double* var)
{
    hipStream_t s = c->stream;
    digest_kernel(c);
    const int64_t N = c->N;
    const int D = c->D;
    PhaseDrain pd(c);
    // the chunk of a query, as kg_impl's candidates (a candidate's answer must not depend on the batch around it)
    const int64_t mc_max = qt_serves(c) ? qt_rows_per_chunk(N, M) : std::min<int64_t>(nm_cols_per_chunk(c->ld, M), kKgNmChunk);
    QtBufs bc = served_layout(c, mc_max, N);
    double *dF = nullptr, *dAdd = nullptr, *dE = nullptr, *dP = nullptr, *dMu = nullptr;
    QueryScratch qs(c);
    if (const int e = qs.carve([&](Carver& cv) {
            qt_carve(bc, cv);
            dF = cv.take<double>((size_t)(2 * std::max<int64_t>(n, 1)));
            dAdd = cv.take<double>((size_t)(2 * mc_max));
            dE = cv.take<double>((size_t)mc_max);
            dP = cv.take<double>((size_t)(4 * mc_max));
            dMu = cv.take<double>((size_t)(2 * mc_max));
        }))
        return e;
    if (n > 0)
        HIPCHK(c, hipMemcpyAsync(dF, front, sizeof(double) * (size_t)(2 * n), hipMemcpyHostToDevice, s));

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
            HIPCHK(c, copy2d_from_host(dAdd, mc_max, mean_add + m0, M, mc, 2, s));
        const int u1 = mk.mark();
        {
            PhaseScope ps(c, GPE_PH_QUERY, 0.0);
            EhviArgs q{};
            q.front = dF;
            q.n = (int)n;
            q.r1 = ref[0];
            q.r2 = ref[1];
            q.mu1 = bc.dKta + (int64_t)out1 * bc.mc_max;
            q.mu2 = bc.dKta + (int64_t)out2 * bc.mc_max;
            q.add1 = mean_add ? dAdd : nullptr;
            q.add2 = mean_add ? dAdd + mc_max : nullptr;
            q.var = bc.dVar;
            q.var_add = var_add;
            q.M = mc;
            q.ehvi = dE;
            q.partials = partials ? dP : nullptr;
            q.ldp = mc_max;
            q.mu_out = mu ? dMu : nullptr;
            q.ldm = mc_max;
            launch_ehvi2(s, q);
        }
        const int u2 = mk.mark();
        if (ehvi)
            HIPCHK(c, hipMemcpyAsync(ehvi + m0, dE, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s));
        if (partials)
            HIPCHK(c, copy2d_to_host(partials + m0, M, dP, mc_max, mc, 4, s));
        if (mu)
            HIPCHK(c, copy2d_to_host(mu + m0, M, dMu, mc_max, mc, 2, s));
        if (var)
            HIPCHK(c, hipMemcpyAsync(var + m0, bc.dVar, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s));
        const int u3 = mk.mark();
        rc = stream_wait(c, "ehvi2_batch", true);
        ms[0] += mk.ms(u0, u1);
        ms[1] += mk.ms(u1, u2);
        ms[2] += mk.ms(u2, u3);
    }
    if (c->prof && rc == GPE_OK)
        for (int q = 0; q < 3; ++q)
            c->ehvi_ms[q] = ms[q];
    return rc;
}

int gpe_ehvi2_batch(gpe_handle c, int out1, int out2, const double* Xc, int64_t M, const double* mean_add, double var_add, const double* front,
                    int64_t n, const double* ref, double* ehvi, double* partials, double* mu, double* var)
{
    if (!c || M < 0 || !(var_add >= 0.0) || !std::isfinite(var_add) || (M > 0 && !Xc) || n > GPE_EHVI_MAX_FRONT || !ehvi_front_ok(front, n, ref))
        return GPE_ERR_ARG;
    if (!c->have_L)
        return GPE_ERR_STATE;
    if (c->host_K)
        return GPE_ERR_UNSUPPORTED;
    if (out1 == out2 || out1 < 0 || out2 < 0 || out1 >= c->P || out2 >= c->P)
        return GPE_ERR_ARG;
    if (M == 0 || (!ehvi && !partials && !mu && !var))
        return GPE_OK;
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    return ehvi_impl(c, out1, out2, Xc, M, mean_add, var_add, front, n, ref, ehvi, partials, mu, var);
}

int gpe_ehvi_phase_ms(gpe_handle c, double* ms3)
{
    if (!c || !ms3)
        return GPE_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    for (int q = 0; q < 3; ++q)
        ms3[q] = c->ehvi_ms[q];
    return GPE_OK;
}
