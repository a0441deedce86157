// qgrad.hpp — the posterior's gradient in the query point over a point batch (include/gpe_query_grad.h): host side.  Kernels: qgrad.hip.
// A part of engine.hip's translation unit (included there, once, behind query.hpp, whose chunk helpers it shares).
#pragma once

// the call's own phases — forward part, backward solve, gradient kernel — for gpe_query_grad_phase_ms: four boundaries per chunk
// (a Marks of its own), added up over the chunks after each chunk's stream wait
static void qg_collect(gpe_ctx* c, const Marks& mk)
{
    for (int q = 0; q < 3; ++q)
        c->qgrad_ms[q] += mk.ms(q, q + 1);
}

// the gradient columns of one chunk: the pass over Wt / alpha, and the results to the caller's arrays
//   Qt: the chunk's SoA points (ldq), Wt: mc x N (ldw) or null; dPartG / dG: scratch (qg_extra)
static void qg_columns(gpe_ctx* c, const double* Qt, int64_t ldq, int64_t mc, int64_t mc_max, const double* Wt, int64_t ldw, int nseg,
                       double* dPartG, double* dG, double* dkta, double* dvar, int64_t m0, int64_t M)
{
    hipStream_t s = c->stream;
    const int D = c->D, P = c->P;
    const int cbeg = dkta ? 0 : P, ncol = (dvar ? P + 1 : P) - cbeg;
    {
        PhaseScope ps(c, GPE_PH_QUERY, (double)c->N * mc * ((double)c->kp.D * (ncol + 1) + 40.0));
        launch_query_grad(s, Qt, ldq, mc, c->dXt, c->ld, c->N, Wt, ldw, c->dAl, c->ld, P, c->kp, lam_params(c), cbeg, ncol, nseg, dPartG, ldq,
                          dG, mc_max);
    }
    if (dkta)
        copy2d_to_host(dkta + m0, M, dG, mc_max, mc, (int64_t)D * P, s);
    if (dvar)
        copy2d_to_host(dvar + m0, M, dG + (int64_t)mc_max * D * (P - cbeg), mc_max, mc, D, s);
}
// scratch of qg_columns behind the chunk buffers, in doubles: the partials, then the folded columns
static void qg_extra(const gpe_ctx* c, int nseg, int64_t ldq, int64_t mc_max, size_t* n_part, size_t* n_g)
{
    *n_part = query_grad_partial_doubles(nseg, c->P + 1, c->kp.D, ldq);
    *n_g = (size_t)mc_max * (size_t)c->D * (size_t)(c->P + 1);
}

// the backward half behind qt_forward, for the mc rows of b.dZt (needs qt_panels)
static void qt_backward(gpe_ctx* c, const QtBufs& b, int64_t mc)
{
    hipStream_t s = c->stream;
    const int64_t N = c->N, ld = c->ld, nbo = NBO, ldq = b.ldq;
    // Wt = Zt L^-1, from the last outer panel to the first; Zt is the running right-hand side (destroyed), Wt goes where
    // Kst was (b.dKst):
    //   Wt[:, p]        = Acc[:, p] X_p                       X_p = inv(L_pp) (qt_panels), untransposed this time
    //   Acc[:, 0 .. o0) -= Wt[:, p] L[p, 0 .. o0)
    // Both products have B with k contiguous: the register-staged matrix-core kernel (the direct-to-LDS one takes
    // operands contiguous along their non-k index only, gemm.hip: glds_ok).
    for (int64_t o0 = (b.npan - 1) * nbo; o0 >= 0; o0 -= nbo) {
        const int64_t pw = std::min<int64_t>(nbo, N - o0);
        {
            GemmArgs g{};
            g.C = b.dKst + o0 * ldq;
            g.ldc = ldq;
            g.A = b.dZt + o0 * ldq;
            g.lda = ldq;
            g.B = b.dXp + (o0 / nbo) * (nbo * nbo);
            g.ldb = nbo;
            g.b_kmajor = 1;
            g.m = mc;
            g.n = pw;
            g.k = pw;
            g.overwrite = 1;
            g.tile = b.qtile;
            PhaseScope ps(c, GPE_PH_QUERY, gemm_flops(g));
            launch_gemm_sub(s, g);
        }
        if (o0 > 0) {
            GemmArgs g{};
            g.tile = b.qtile;
            g.C = b.dZt;
            g.ldc = ldq;
            g.A = b.dKst + o0 * ldq;
            g.lda = ldq;
            g.B = c->dA + o0;
            g.ldb = ld;
            g.b_kmajor = 1;
            g.m = mc;
            g.n = o0;
            g.k = pw;
            PhaseScope ps(c, GPE_PH_QUERY, gemm_flops(g));
            launch_gemm_sub(s, g);
        }
    }
}

// kta and var by the chunk steps of the batched query, then Wt = Kst K^-1 (mc x N, the points contiguous) for the variance's gradient:
//   transposed layout: Wt = Zt L^-1 (qt_backward) into the buffer Kst occupied;
//   else: one product with K^-1 (ensure_inv, cached on the handle until K changes; a symmetric copy of its lower triangle) of a
//   second cross kernel, built with the points contiguous
static int qgrad_impl(gpe_ctx* c, const double* Xq, int64_t M, double* kta, double* var, double* dkta, double* dvar)
{
    hipStream_t s = c->stream;
    const int64_t N = c->N, ld = c->ld;
    const int D = c->D;
    const bool transposed = qt_enabled(c);
    if (dvar && !transposed) {
        const int e = ensure_inv(c);
        if (e)
            return e;
    }
    PhaseDrain pd(c);
    const int64_t mc_max = transposed ? qt_rows_per_chunk(N, M) : nm_cols_per_chunk(ld, M);
    QtBufs b = transposed ? qt_layout(c, mc_max, N) : nm_layout(c, mc_max, false);
    const int64_t ldt = transposed ? b.ldq : mc_max + 16; // Wt's leading dimension
    const bool grads = dkta || dvar, want_z = var || (transposed && dvar), want_ks = transposed || kta || var;
    const size_t n_t = dvar && !transposed ? (size_t)(ldt * N) : 0, n_ki = dvar && !transposed ? (size_t)(ld * N) : 0;
    size_t n_partg = 0, n_g = 0;
    if (grads)
        qg_extra(c, b.nseg, ldt, mc_max, &n_partg, &n_g);
    double *dKst2 = nullptr, *dWt = nullptr, *dKi = nullptr, *dPartG = nullptr, *dG = nullptr;
    QueryScratch qs(c);
    if (const int e = qs.carve([&](Carver& cv) {
            qt_carve(b, cv);
            dKst2 = cv.take<double>(n_t); // the cross kernel with the points contiguous
            dWt = cv.take<double>(n_t);
            dKi = cv.take<double>(n_ki);
            dPartG = cv.take<double>(n_partg);
            dG = cv.take<double>(n_g);
        }))
        return e;
    if (n_ki)
        kinv_operand(c, dKi);
    chunk_begin(c, b, want_z);
    int rc = GPE_OK;
    for (int64_t m0 = 0; m0 < M && rc == GPE_OK; m0 += mc_max) {
        const int64_t mc = std::min<int64_t>(mc_max, M - m0);
        Marks mk(c->pool, s, c->prof);
        mk.mark();
        chunk_head(c, b, Xq + m0 * D, true, mc, want_ks, kta != nullptr, kta, m0, M);
        ZView z;
        if (want_z)
            z = chunk_solve(c, b, mc);
        if (var) { // (before Zt is consumed below)
            chunk_var(c, b, mc, z);
            hipMemcpyAsync(var + m0, b.dVar, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s);
        }
        mk.mark();
        const double* Wt = nullptr;
        if (dvar && transposed) {
            qt_backward(c, b, mc);
            Wt = b.dKst;
        }
        else if (dvar) {
            {
                PhaseScope ps(c, GPE_PH_QUERY, 0.0);
                launch_build_Ks(s, b.dQt, b.ldq, mc, c->dXt, ld, N, c->kp, dKst2, ldt); // k is symmetric: the transposed block
            }
            times_kinv(c, dKi, dKst2, dWt, ldt, mc);
            Wt = dWt;
        }
        mk.mark();
        if (grads)
            qg_columns(c, b.dQt, b.ldq, mc, mc_max, Wt, ldt, b.nseg, dPartG, dG, dkta, dvar, m0, M);
        mk.mark();
        rc = stream_wait(c, "query_batch_grad", true);
        qg_collect(c, mk);
    }
    return rc;
}

int gpe_query_batch_grad(gpe_handle c, const double* Xq, int64_t M, double* kta, double* var, double* dkta, double* dvar)
{
    if (!c || M < 0 || (M > 0 && !Xq))
        return GPE_ERR_ARG;
    if (!c->have_L)
        return GPE_ERR_STATE;
    if (c->host_K)
        return GPE_ERR_UNSUPPORTED;
    if (M == 0 || (!kta && !var && !dkta && !dvar))
        return GPE_OK;
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    digest_kernel(c);
    for (double& ms : c->qgrad_ms)
        ms = 0.0;
    return qgrad_impl(c, Xq, M, kta, var, dkta, dvar);
}

int gpe_query_grad_phase_ms(gpe_handle c, double* ms3) { return phase_ms_get(c, &gpe_ctx::qgrad_ms, ms3); }
