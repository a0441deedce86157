// query.hpp — the batched query (gp.hpp:613-632 for M points): transposed layout for device kernels, the N x M layout for caller-supplied cross kernels, the one-launch paths for a handful of points.
// A part of engine.hip's translation unit (included there, once, at the place its contents used to stand: they share the
// file-local types and helpers of the engine — gpe_ctx, PhaseScope, DevGuard ...); split out in round 6 for readability.
#pragma once

// The batched query (gp.hpp:613-632 for M points) with the POINTS along the contiguous axis.
//   Kst[m + i ldq] = k(x_i, v_m)  (the cross kernel, transposed);   Zt = Kst L^-T, panel by panel:
//     Zt[:, p]       = Acc[:, p] X_p^T                      X_p = inv(L_pp), all panels by one launch (inv.hip)
//     Acc[:, p+1 ..] -= Zt[:, p] L[p+1 .., p]^T             k = the panel width
//   var[m] = k(v_m, v_m) - sum_i Zt[m, i]^2,   kta[m, p] = sum_i Kst[m, i] alpha[i, p].
// In this layout EVERY product is C (-)= A B^T with both operands contiguous along their non-k index — the operand form
// of the direct-to-LDS matrix-core kernel (gemm.hip, k_gemm_glds), as K^-1's U = L^-T (ensure_inv).  The N x M layout
// (rounds 1-2, still the path for caller-supplied cross kernels) has the right-hand sides k-contiguous and ran its
// M N^2 flops through the register-staged kernel: 38 TFLOP/s at N = 16384 against the 53 of the factorisation's updates.
// The buffers of one chunk of <= mc_max points, carved from gpe_ctx::dQuery, and the launches that fill them — shared by
// query_transposed (the marginals) and the joint posterior (joint.hpp), which keeps Zt for all its points at once.
struct QtBufs {
    int64_t mc_max = 0, ldq = 0, npan = 0, zcols = 0;
    int nseg = 1, qtile = 128;
    size_t n_qrm = 0, n_qt = 0, n_kst = 0, n_zt = 0, n_xp = 0, n_part = 0, n_kta = 0, doubles = 0;
    double *dQrm = nullptr, *dQt = nullptr, *dKst = nullptr, *dZt = nullptr, *dXp = nullptr, *dPart = nullptr, *dKta = nullptr, *dVar = nullptr,
           *dKvv = nullptr;
};
// mc_max: points per chunk (a multiple of 64); zcols >= N: columns of Zt (the joint posterior pads its k range with zero columns)
// N_ (>= 0): size for that many samples instead of the handle's current count (the blocked append reserves for its last chunk)
static QtBufs qt_layout(const gpe_ctx* c, int64_t mc_max, int64_t zcols, int64_t N_ = -1)
{
    QtBufs b;
    const int64_t N = N_ >= 0 ? N_ : c->N, nbo = c->nbo;
    const int D = c->D, P = c->P;
    b.mc_max = mc_max;
    b.ldq = mc_max + 16; // not a power of two (HBM channel camping on column strides), even, 16-byte rows
    b.npan = (N + nbo - 1) / nbo;
    b.zcols = zcols;
    b.nseg = (int)std::max<int64_t>(1, std::min<int64_t>(32, N / 512));
    b.n_qrm = (size_t)(mc_max * std::max(D, 1));
    b.n_qt = (size_t)(b.ldq * std::max(xt_rows(D), 1));
    b.n_kst = (size_t)(b.ldq * N);
    b.n_zt = (size_t)(b.ldq * zcols);
    b.n_xp = (size_t)(b.npan * nbo * nbo);
    b.n_part = (size_t)b.nseg * std::max(P, 1) * (size_t)b.ldq;
    b.n_kta = (size_t)(mc_max * P);
    b.doubles = b.n_qrm + b.n_qt + b.n_kst + b.n_zt + b.n_xp + b.n_part + b.n_kta + 2 * (size_t)mc_max;
    // The tile of every product below is picked from N alone, never from the batch: the 128 x 128 and the 64 x 64 kernels round
    // differently in the last bit (measured, round 6: a point's variance moved by 1.5e-15 with the size of the batch it was asked
    // in, because launch_gemm_sub picks the tile from the live-tile count = from mc).  A point's answer must not depend on the
    // batch around it (tests/test_gpu_configs.py: the 100 000-point batch of configs[2] bitwise equal to chunks of 4096).
    b.qtile = N >= 1024 ? 128 : 64;
    return b;
}
static void qt_carve(QtBufs& b, double* base)
{
    b.dQrm = base;
    b.dQt = b.dQrm + b.n_qrm;
    b.dKst = b.dQt + b.n_qt; // the cross kernel, then the running right-hand side Acc
    b.dZt = b.dKst + b.n_kst;
    b.dXp = b.dZt + b.n_zt;
    b.dPart = b.dXp + b.n_xp;
    b.dKta = b.dPart + b.n_part;
    b.dVar = b.dKta + b.n_kta;
    b.dKvv = b.dVar + b.mc_max;
}
// grow gpe_ctx::dQuery to `bytes` (contents are not kept)
static int query_reserve(gpe_ctx* c, size_t bytes)
{
    HIPCHK(c, c->dQuery.reserve((bytes + sizeof(double) - 1) / sizeof(double)));
    return GPE_OK;
}
static void query_release(gpe_ctx* c)
{
    if (sizeof(double) * c->dQuery.capacity() > ((size_t)64 << 20)) // a large batch: give the memory back
        c->dQuery.reset();
}
// X_p of every panel, compact (in front of the first chunk whose Zt is wanted)
static void qt_panels(gpe_ctx* c, const QtBufs& b)
{
    PhaseScope ps(c, GPE_PH_QUERY, 0.0);
    launch_inv_panels(c->stream, c->dA, c->ld, c->N, (int)c->nbo, c->dXinv, b.dXp, 0, nullptr, 0);
}
// Zt = Kst L^-T for the mc rows of b.dKst — a chunk's cross kernel, or right-hand sides a caller put in its place (pathwise.hpp);
// Kst is destroyed
static void qt_forward(gpe_ctx* c, const QtBufs& b, int64_t mc)
{
    hipStream_t s = c->stream;
    const int64_t N = c->N, ld = c->ld, nbo = c->nbo, ldq = b.ldq;
    double *dKst = b.dKst, *dZt = b.dZt;
    for (int64_t o0 = 0; o0 < N; o0 += nbo) { // gp.hpp:620, transposed
        const int64_t pw = std::min<int64_t>(nbo, N - o0), oe = o0 + pw;
        {
            GemmArgs g{};
            g.C = dZt + o0 * ldq;
            g.ldc = ldq;
            g.A = dKst + o0 * ldq;
            g.lda = ldq;
            g.B = b.dXp + (o0 / nbo) * (nbo * nbo);
            g.ldb = nbo;
            g.m = mc;
            g.n = pw;
            g.k = pw;
            g.overwrite = 1;
            g.tile = b.qtile;
            PhaseScope ps(c, GPE_PH_QUERY, gemm_flops(g));
            launch_gemm_sub(s, g);
        }
        if (oe < N) {
            GemmArgs g{};
            g.tile = b.qtile;
            g.C = dKst + oe * ldq;
            g.ldc = ldq;
            g.A = dZt + o0 * ldq;
            g.lda = ldq;
            g.B = c->dA + oe + o0 * ld;
            g.ldb = ld;
            g.m = mc;
            g.n = N - oe;
            g.k = pw;
            PhaseScope ps(c, GPE_PH_QUERY, gemm_flops(g));
            launch_gemm_sub(s, g);
        }
    }
}
// one chunk of mc points (host, row-major): the points, Kst, kta (on the device and, kta != null, to kta[m0 + p M]) and,
// want_z, Zt = Kst L^-T (Kst is destroyed)
static void qt_chunk(gpe_ctx* c, const QtBufs& b, const double* Xq_chunk, int64_t mc, bool want_kta, double* kta, int64_t m0, int64_t M,
                     bool want_z)
{
    hipStream_t s = c->stream;
    const int64_t N = c->N, ld = c->ld, ldq = b.ldq;
    const int D = c->D, P = c->P;
    double* dKst = b.dKst;
    hipMemcpyAsync(b.dQrm, Xq_chunk, sizeof(double) * (size_t)(mc * D), hipMemcpyHostToDevice, s);
    launch_transpose_x(s, b.dQrm, mc, D, b.dQt, ldq, 0);
    project_lambda(c, s, b.dQt, ldq, 0, mc);
    {
        // k is symmetric: the cross kernel with the roles of samples and points exchanged IS the transposed block
        PhaseScope ps(c, GPE_PH_QUERY, 0.0);
        launch_build_Ks(s, b.dQt, ldq, mc, c->dXt, ld, N, c->kp, dKst, ldq); // gp.hpp:626-632
    }
    if (want_kta) {
        PhaseScope ps(c, GPE_PH_QUERY, 2.0 * N * mc * P);
        launch_kta_t(s, dKst, ldq, N, mc, c->dAl, ld, P, b.dKta, b.mc_max, b.dPart, ldq, b.nseg); // gp.hpp:615
        if (kta)
            for (int p = 0; p < P; ++p)
                hipMemcpyAsync(kta + m0 + (int64_t)p * M, b.dKta + (int64_t)p * b.mc_max, sizeof(double) * (size_t)mc,
                               hipMemcpyDeviceToHost, s);
    }
    if (!want_z)
        return;
    qt_forward(c, b, mc);
}

static int query_transposed(gpe_ctx* c, const double* Xq, int64_t M, double* kta, double* var)
{
    hipStream_t s = c->stream;
    const int64_t N = c->N;
    const int D = c->D;
    // chunk: two ldq x N buffers of <= 2 GiB each
    int64_t mc_max = std::max<int64_t>(64, (((int64_t)1 << 28) / std::max<int64_t>(N, 1)) / 64 * 64);
    mc_max = std::min<int64_t>(mc_max, round_up(M, 64));
    QtBufs b = qt_layout(c, mc_max, N);
    {
        const int e = query_reserve(c, sizeof(double) * b.doubles);
        if (e)
            return e;
    }
    qt_carve(b, c->dQuery);
    int rc = GPE_OK;
    if (var)
        qt_panels(c, b);
    for (int64_t m0 = 0; m0 < M && rc == GPE_OK; m0 += mc_max) {
        const int64_t mc = std::min<int64_t>(mc_max, M - m0);
        qt_chunk(c, b, Xq + m0 * D, mc, kta != nullptr, kta, m0, M, var != nullptr);
        if (var) {
            PhaseScope ps(c, GPE_PH_QUERY, 2.0 * N * mc);
            launch_kvv(s, b.dQt, b.ldq, mc, c->kp, b.dKvv);
            launch_row_var_t(s, b.dZt, b.ldq, N, mc, b.dKvv, b.dVar, b.dPart, b.ldq, b.nseg); // gp.hpp:621
            hipMemcpyAsync(var + m0, b.dVar, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s);
        }
        if (hipStreamSynchronize(s) != hipSuccess) {
            c->err = "query_batch: stream sync failed";
            rc = GPE_ERR_HIP;
        }
    }
    drain_phases(c);
    query_release(c);
    return rc;
}

// shared by gpe_query_batch (cross kernel built on the device from Xq) and gpe_query_batch_cross
// (cross kernel handed over by the caller): kta = Ks^T alpha, var = kvv - colsum((L^-1 Ks)^2)
static int query_impl(gpe_ctx* c, const double* Xq, const double* KsHost, int64_t M, double* kta, double* var)
{
    hipStream_t s = c->stream;
    digest_kernel(c);
    const int64_t N = c->N, ld = c->ld;
    const int D = c->D, P = c->P;
    if (c->small_path && Xq && N <= small_max_n() && M <= 8 && (int64_t)M * D <= 1024 && P <= GPE_MAX_P) {
        // the per-point query of an acquisition functor on a small GP: one launch (one workgroup per point), the
        // points read from and the results written to pinned host memory (small.hip)
        memcpy(c->hSmall + 256, Xq, sizeof(double) * (size_t)(M * D));
        SmallQueryArgs q{};
        q.L = c->dA;
        q.ld = ld;
        q.Xinv = c->dXinv;
        q.Xt = c->dXt;
        q.ldx = ld;
        q.Al = c->dAl;
        q.P = P;
        q.n = (int)N;
        q.M = (int)M;
        q.D = D;
        q.xq_host = c->hSmall + 256;
        q.kta_host = c->hSmall + 16;
        q.var_host = c->hSmall + 16 + 8 * GPE_MAX_P;
        q.seq = c->hSmallSeq;
        q.seq_val = ++c->small_seq;
        q.want_kta = kta ? 1 : 0;
        q.want_var = var ? 1 : 0;
        {
            PhaseScope ps(c, GPE_PH_QUERY, (double)N * N * M);
            launch_small_query(s, q, c->kp, lam_params(c));
        }
        ++c->small_calls;
        int rc = small_wait(c, (int)M, q.seq_val);
        drain_phases(c);
        if (rc)
            return rc;
        if (kta)
            memcpy(kta, q.kta_host, sizeof(double) * (size_t)(M * P));
        if (var)
            memcpy(var, q.var_host, sizeof(double) * (size_t)M);
        return GPE_OK;
    }
    // a handful of points (the per-point calls of an acquisition functor, gp.hpp:159-191): the forward
    // substitution runs as ONE data-flow launch (k_trsv_fwd_flow, <= GPE_MAX_P right-hand sides) instead of a
    // blocked matrix solve, whose ~2 N/64 dependent matrix-core launches are all launch floor there
    static const bool sweep_ok = env_not_zero("GPE_QUERY_SWEEP");
    static const bool transposed_ok = env_not_zero("GPE_QUERY_T");
    const bool few = sweep_ok && c->flow_solve && M <= GPE_MAX_P && (N + NB - 1) / NB <= 256;
    if (Xq && !few && transposed_ok && c->nbo % 128 == 0 && c->nbo <= 256 && N >= c->nbo)
        return query_transposed(c, Xq, M, kta, var);
    // chunk so that the N x mc cross matrix stays under ~2 GiB
    int64_t mc_max = std::max<int64_t>(64, ((int64_t)1 << 28) / std::max<int64_t>(ld, 1));
    mc_max = round_up(std::min<int64_t>(mc_max, round_up(M, 64)), 64);
    if (few)
        mc_max = GPE_MAX_P;
    const int64_t ldq = mc_max;
    // one allocation, carved up; kept across calls while small so that point queries do not malloc/free
    const size_t n_qrm = (size_t)(mc_max * std::max(D, 1)), n_qt = (size_t)(ldq * std::max(xt_rows(D), 1));
    const size_t n_ks = (size_t)(ld * mc_max), n_z = few ? n_ks : 0, n_kta = (size_t)(mc_max * P);
    const size_t need = sizeof(double) * (n_qrm + n_qt + n_ks + n_z + n_kta + 2 * (size_t)mc_max);
    {
        const int e = query_reserve(c, need);
        if (e)
            return e;
    }
    double* dQrm = c->dQuery;
    double* dQt = dQrm + n_qrm;
    double* dKs = dQt + n_qt;
    double* dZ = dKs + n_ks;
    double* dKta = dZ + n_z;
    double* dVar = dKta + n_kta;
    double* dKvv = dVar + mc_max;
    int rc = GPE_OK;
    for (int64_t m0 = 0; m0 < M && rc == GPE_OK; m0 += mc_max) {
        const int64_t mc = std::min<int64_t>(mc_max, M - m0);
        if (Xq) {
            hipMemcpyAsync(dQrm, Xq + m0 * D, sizeof(double) * (size_t)(mc * D), hipMemcpyHostToDevice, s);
            launch_transpose_x(s, dQrm, mc, D, dQt, ldq, 0);
            project_lambda(c, s, dQt, ldq, 0, mc);
            PhaseScope ps(c, GPE_PH_QUERY, 0.0);
            launch_build_Ks(s, c->dXt, ld, N, dQt, ldq, mc, c->kp, dKs, ld); // gp.hpp:626-632
        }
        else {
            copy2d_from_host(dKs, ld, KsHost + m0 * N, N, N, mc, s);
        }
        if (kta) {
            PhaseScope ps(c, GPE_PH_QUERY, 2.0 * N * mc * P);
            launch_kta(s, dKs, ld, N, mc, c->dAl, ld, P, dKta, mc_max); // gp.hpp:615
            for (int p = 0; p < P; ++p)
                hipMemcpyAsync(kta + m0 + (int64_t)p * M, dKta + (int64_t)p * mc_max, sizeof(double) * (size_t)mc,
                               hipMemcpyDeviceToHost, s);
        }
        if (var) {
            const double* Z = dKs;
            if (few) {
                PhaseScope ps(c, GPE_PH_QUERY, (double)N * N * mc);
                launch_trsv_fwd_flow(s, c->dA, ld, N, c->dXinv, dKs, ld, dZ, ld, (int)mc, c->dInfo + 1); // gp.hpp:620
                Z = dZ;
            }
            else
                trsm_left_blocked(c, c->dA, dKs, ld, N, mc, false, GPE_PH_QUERY); // gp.hpp:620
            PhaseScope ps(c, GPE_PH_QUERY, 2.0 * N * mc);
            if (Xq)
                launch_kvv(s, dQt, ldq, mc, c->kp, dKvv);
            else
                hipMemsetAsync(dKvv, 0, sizeof(double) * (size_t)mc, s);
            launch_col_var(s, Z, ld, N, mc, dKvv, dVar); // gp.hpp:621
            hipMemcpyAsync(var + m0, dVar, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s);
        }
        if (hipStreamSynchronize(s) != hipSuccess) {
            c->err = "query_batch: stream sync failed";
            rc = GPE_ERR_HIP;
        }
        else if (few && var && flow_failed(c)) {
            // the one-launch sweep gave up (never expected): the same chunk through the blocked solve, in place
            trsm_left_blocked(c, c->dA, dKs, ld, N, mc, false, GPE_PH_QUERY);
            launch_col_var(s, dKs, ld, N, mc, dKvv, dVar);
            hipMemcpyAsync(var + m0, dVar, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s);
            if (hipStreamSynchronize(s) != hipSuccess) {
                c->err = "query_batch: stream sync failed";
                rc = GPE_ERR_HIP;
            }
        }
    }
    drain_phases(c);
    query_release(c);
    return rc;
}
