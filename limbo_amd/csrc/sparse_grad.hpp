// sparse_grad.hpp — the analytic gradient of the sparse pseudo-input GP (include/gpe_sparse_grad.h; spgp.hpp:500-580): host side.
// Kernels: sparse_grad.hip.  A part of engine.hip's translation unit, included behind sparse.hpp, whose types and helpers it uses.
#pragma once

extern "C++" {
namespace {

// One device block per handle (gpe_sp_ctx::dGrad), carved per call (V of a chunk lives in the inner context's query scratch, as in
// gpe_sp_compute).  Matrices are Mq x Mq with Mq = M rounded up to 128 and the chunk's buffers ldq x Mq with ldq = the chunk rounded up to 128, both zero-filled once per call: the products run their k range
// over the padded order (k a multiple of 32: the direct-to-LDS kernels), and whole tiles may be read.
struct SpGradBufs {
    int64_t Mq = 0, ldq = 0;
    double *Wl, *IQm, *IAm, *TT, *LiT, *LtiT, *Lmi, *b1, *Kt, *B1t, *IQt, *ILVt, *Qt, *rs, *big, *R, *Racc, *Rpart, *part, *tb, *cs, *dxb, *dhp;
    size_t doubles = 0;
};

SpGradBufs sp_grad_carve(double* base, int64_t M, int64_t N, int D, int P, int64_t chunk, int S0)
{
    SpGradBufs b;
    b.Mq = round_up(M, 128);
    b.ldq = round_up(chunk, 128);
    const int64_t nchunks = (N + chunk - 1) / chunk, ncol = 2 * D + 1;
    size_t off = 0;
    auto take = [&](double** p, int64_t n) {
        *p = base ? base + off : nullptr;
        off += (size_t)round_up(n, 64);
    };
    take(&b.Wl, b.Mq * b.Mq);
    take(&b.IQm, b.Mq * b.Mq);
    take(&b.IAm, b.Mq * b.Mq);
    take(&b.TT, b.Mq * b.Mq);
    take(&b.LiT, b.Mq * b.Mq);
    take(&b.LtiT, b.Mq * b.Mq);
    take(&b.Lmi, b.Mq * b.Mq);
    take(&b.b1, b.Mq * P);
    take(&b.Kt, b.ldq * b.Mq);
    take(&b.B1t, b.ldq * b.Mq);
    take(&b.IQt, b.ldq * b.Mq);
    take(&b.ILVt, b.ldq * b.Mq);
    take(&b.Qt, b.ldq * std::max(xt_rows(D), 1));
    take(&b.rs, b.ldq);
    take(&b.big, b.ldq);
    take(&b.R, b.ldq * P);
    take(&b.Racc, b.Mq * ncol);
    take(&b.Rpart, (int64_t)S0 * b.Mq * ncol);
    take(&b.part, 3 * (N / 64 + nchunks + 1));
    take(&b.tb, b.Mq * D);
    take(&b.cs, 4 * b.Mq);
    take(&b.dxb, M * D);
    take(&b.dhp, D + 2);
    b.doubles = off;
    return b;
}

int64_t sp_grad_chunk(int64_t M, int64_t N)
{
    int64_t ch = sparse_grad_default_chunk(M);
    if (const char* e = getenv("GPE_SPARSE_CHUNK")) { // (as sp_chunk: read per call)
        const long long v = atoll(e);
        if (v > 0)
            ch = round_up((int64_t)v, 64);
    }
    return std::min<int64_t>(ch, round_up(N, 64));
}

// C (lower, then symmetrised) = X^T X for the lower triangular X (order M, both ldm): K^-1 = L^-T L^-1 as ensure_inv forms it
void sp_grad_lauum(hipStream_t s, const double* X, double* C, int64_t ldm, int64_t M)
{
    GemmArgs g{};
    g.C = C;
    g.ldc = ldm;
    g.A = X;
    g.lda = ldm;
    g.a_kmajor = 1;
    g.B = X;
    g.ldb = ldm;
    g.b_kmajor = 1;
    g.m = g.n = g.k = M;
    g.tri = 1;
    g.ktri = 1;
    g.overwrite = 1;
    launch_gemm_sub(s, g);
    launch_symmetrize_from_lower(s, C, ldm, M);
}

int sp_grad_locked(gpe_sp_ctx* h, double* d_xb, double* d_hp)
{
    if (!h->computed)
        return GPE_ERR_STATE;
    gpe_ctx *in = h->in, *sc = h->sc;
    const int64_t N = h->N, M = h->M, Mpad = h->Mpad;
    const int D = h->D, P = h->P;
    std::lock_guard<std::mutex> lk(in->mu);
    hipStream_t s = in->stream;
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, in->device);
    const int64_t chunk = sp_grad_chunk(M, N);
    const bool own_gram = sp_use_gram_kernel(M, cus);
    const int SR0 = sparse_grad_row_slices(M, std::min(chunk, N), cus); // (the first chunk is the longest)
    SpGradBufs b = sp_grad_carve(nullptr, M, N, D, P, chunk, SR0);
    HIPCHK(h, h->dGrad.reserve((size_t)b.doubles));
    b = sp_grad_carve(h->dGrad, M, N, D, P, chunk, SR0);
    const int64_t Mq = b.Mq, ldq = b.ldq, pstride = Mpad * Mpad;
    const int SG0 = sparse_gram_slices(M, std::min(chunk, N), cus);
    std::vector<int64_t> plan;
    if (own_gram) {
        const int64_t rows = sparse_gram_plan(M, N, chunk, cus, nullptr, 0);
        plan.resize((size_t)rows * 5);
        (void)sparse_gram_plan(M, N, chunk, cus, plan.data(), rows);
        HIPCHK(h, h->dPlan.reserve((size_t)(rows * 5)));
        if (SG0 > 1)
            HIPCHK(h, h->dPart.reserve((size_t)(SG0 * pstride)));
        HIPCHK(h, hipMemcpyAsync(h->dPlan, plan.data(), sizeof(int64_t) * plan.size(), hipMemcpyHostToDevice, s));
    }
    // two boundaries around the M x M part, per chunk two around each of its three phases, two around the finish
    Marks mk(in->pool, s, h->prof);
    hipEvent_t ev_order[2] = {nullptr, nullptr};
    // ---- M x M: Li = L^-1, invQ = Li^T Li; Lmi = Lm^-1; Lti = Lm^-1 Li = (L Lm)^-1, invA = Lti^T Lti (spgp.hpp:501-505), b1 = Lti^T bet
    // (:507); Li^T and Lti^T as matrices of their own: the chunk's products want both operands contiguous along their non-k index
    mk.mark();
    HIPCHK(h, hipMemsetAsync(b.Wl, 0, sizeof(double) * (size_t)(7 * Mq * Mq), s)); // Wl, IQm, IAm, TT, LiT, LtiT, Lmi
    HIPCHK(h, hipMemsetAsync(b.Kt, 0, sizeof(double) * (size_t)(4 * ldq * Mq), s)); // Kt, B1t, IQt, ILVt
    launch_set_identity(s, b.Wl, Mq, M);
    launch_set_identity(s, b.Lmi, Mq, M);
    trsm_left_blocked(in, in->dA, b.Wl, Mq, M, M, true, GPE_PH_INV);
    sp_grad_lauum(s, b.Wl, b.IQm, Mq, M);
    launch_sp_gtrans(s, b.Wl, b.LiT, Mq, M);
    {
        // the solves with Lm go to the scratch context's stream (the blocked solve launches on its context's): ordered by events
        hipEvent_t e0 = get_event(in), e1 = get_event(in);
        hipEventRecord(e0, s);
        hipStreamWaitEvent(sc->stream, e0, 0);
        trsm_left_blocked(sc, sc->dA, b.Wl, Mq, M, M, true, GPE_PH_INV);
        trsm_left_blocked(sc, sc->dA, b.Lmi, Mq, M, M, true, GPE_PH_INV);
        hipEventRecord(e1, sc->stream);
        hipStreamWaitEvent(s, e1, 0);
        ev_order[0] = e0;
        ev_order[1] = e1;
    }
    sp_grad_lauum(s, b.Wl, b.IAm, Mq, M);
    launch_sp_gtrans(s, b.Wl, b.LtiT, Mq, M);
    launch_sp_gb1(s, b.Wl, Mq, M, h->dBet, Mpad, P, b.b1, Mq);
    mk.mark();
    // ---- the pass over N.  V of a chunk comes from the model's own path (sp_v_chunk: the cross kernel and the solve exactly as
    // gpe_sp_compute ran them): ep, Lm and bet were formed from THAT V, and the gradient's large terms cancel only against a V that
    // is consistent with them — K~ through explicit inverses instead lost three digits at M = 1024 (cond K_mm 7e7).
    QtBufs bq = sp_layout(in, chunk);
    QueryScratch qs(in);
    if (const int e = qs.carve(bq)) {
        h->err = "sparse GP gradient: " + in->err;
        return e;
    }
    chunk_begin(in, bq, true);
    const int64_t nt = (M + 63) / 64, tiles = nt * (nt + 1) / 2;
    int64_t row0 = 0, slot0 = 0, blk0 = 0;
    for (int64_t n0 = 0; n0 < N; n0 += chunk) {
        const int64_t mc = std::min<int64_t>(chunk, N - n0);
        mk.mark();
        const ZView z = sp_v_chunk(h, bq, h->dX + n0 * D, mc); // V (:396-398)
        launch_sp_grs(s, h->dEp + n0, mc, b.rs);
        launch_sp_gvt(s, z.p, z.sm(), z.si(), mc, M, b.rs, b.B1t, ldq); // V~^T (:401), for now where B1t will be
        for (int q = 0; q < 3; ++q) { // ILVt = V~t Lm^-T (:483), IQt = V~t L^-1 (:504 invLV), B1t = ILVt Lt^-1 (:502)
            GemmArgs g{};
            g.C = q == 0 ? b.ILVt : q == 1 ? b.IQt : b.B1t;
            g.ldc = ldq;
            g.A = q == 2 ? b.ILVt : b.B1t;
            g.lda = ldq;
            g.B = q == 0 ? b.Lmi : q == 1 ? b.LiT : b.LtiT; // C = A B^T
            g.ldb = Mq;
            g.m = mc;
            g.n = M;
            g.k = Mq; // (the operands' columns M .. Mq are zero)
            g.overwrite = 1;
            launch_gemm_sub(s, g);
        }
        launch_transpose_x(s, h->dX + n0 * D, mc, D, b.Qt, ldq, 0);
        launch_build_Ks(s, b.Qt, ldq, mc, in->dXt, in->ld, M, in->kp, b.Kt, ldq); // K(Xb, X)^T (:396), transposed layout
        launch_sp_scale(s, b.Kt, 1, ldq, mc, M, b.rs, b.Kt); // K~ (:400)
        mk.mark();
        mk.mark();
        launch_sp_gcol(s, b.ILVt, b.IQt, ldq, mc, M, h->dBet, Mpad, P, h->dY + n0, N, h->dEp + n0, b.rs, h->c, h->sig, h->jitter, b.big, b.R,
                       b.part + 3 * blk0);
        blk0 += (mc + 63) / 64;
        launch_sp_grow(s, b.Kt, b.B1t, b.IQt, ldq, mc, M, b.b1, Mq, P, b.big, b.R, b.Qt, in->kp, h->sig, sparse_grad_row_slices(M, mc, cus), b.Rpart,
                       Mq, n0 == 0 ? 1 : 0, b.Racc);
        mk.mark();
        mk.mark();
        if (own_gram) { // TT += IQ diag(bigsum) IQ^T (:518): the model's Gram kernel, signed weights
            const int S = sparse_gram_slices(M, mc, cus);
            const int64_t rows = tiles * S;
            if (S == 1)
                launch_sp_gram(s, b.IQt, 1, ldq, b.big, n0, M, h->dPlan + row0 * 5, rows, slot0, b.TT, Mq, 0, n0 == 0 ? 1 : 2);
            else {
                launch_sp_gram(s, b.IQt, 1, ldq, b.big, n0, M, h->dPlan + row0 * 5, rows, slot0, h->dPart, Mpad, pstride, 0);
                launch_sp_fold(s, h->dPart, Mpad, pstride, S, n0 == 0 ? 1 : 0, M, b.TT, Mq);
            }
            row0 += rows;
            slot0 += S;
        }
        else { // the composed path: the weighted copy goes where B1t was (k_sp_grow is done with it)
            launch_sp_scale(s, b.IQt, 1, ldq, mc, M, b.big, b.B1t);
            GemmArgs g{};
            g.C = b.TT;
            g.ldc = Mq;
            g.A = b.B1t;
            g.B = b.IQt;
            g.lda = g.ldb = ldq;
            g.a_kmajor = g.b_kmajor = 1;
            g.m = g.n = M;
            g.k = mc;
            g.tri = 1;
            g.overwrite = 2;
            launch_gemm_sub(s, g);
        }
        mk.mark();
    }
    mk.mark();
    launch_symmetrize_from_lower(s, b.TT, Mq, M);
    launch_sp_gfinish(s, in->dXt, in->ld, in->kp, M, P, b.b1, Mq, b.IQm, b.IAm, b.TT, Mq, b.Racc, h->sig, h->jitter, b.part, blk0, b.dxb, b.tb, b.cs,
                      b.dhp);
    mk.mark();
    std::vector<double> hxb((size_t)(M * D)), hhp((size_t)D + 2);
    HIPCHK(h, hipMemcpyAsync(hxb.data(), b.dxb, sizeof(double) * hxb.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(hhp.data(), b.dhp, sizeof(double) * hhp.size(), hipMemcpyDeviceToHost, s));
    const bool sync_ok = hipStreamSynchronize(s) == hipSuccess && hipGetLastError() == hipSuccess;
    in->pool.push_back(ev_order[0]);
    in->pool.push_back(ev_order[1]);
    if (!sync_ok) {
        h->err = "sparse GP gradient: stream sync failed";
        return GPE_ERR_HIP;
    }
    if (h->prof) {
        const int n = mk.count();
        for (double& ms : h->gms)
            ms = 0.0;
        h->gms[0] = mk.ms(0, 1);
        for (int q = 2; q + 5 < n - 2; q += 6) // (the chunks' six boundaries each, between the first two and the last two)
            for (int ph = 1; ph <= 3; ++ph)
                h->gms[ph] += mk.ms(q + 2 * ph - 2, q + 2 * ph - 1);
        h->gms[4] = mk.ms(n - 2, n - 1);
    }
    if (d_xb)
        memcpy(d_xb, hxb.data(), sizeof(double) * hxb.size());
    memcpy(d_hp, hhp.data(), sizeof(double) * hhp.size());
    return GPE_OK;
}

} // namespace
} // extern "C++"

int gpe_sp_grad(gpe_sp_handle h, double* d_xb, double* d_hp)
{
    if (!h || !d_hp)
        return GPE_ERR_ARG;
    SpDevGuard g(h);
    std::lock_guard<std::mutex> lk(h->mu);
    return sp_grad_locked(h, d_xb, d_hp);
}

int gpe_sp_objective_grad(gpe_sp_handle h, const double* Xb, const double* log_b, double log_c, double log_sig, double jitter, double* nlml,
                          double* d_xb, double* d_hp)
{
    if (!h || !nlml || !d_hp)
        return GPE_ERR_ARG;
    int rc = GPE_OK;
    if (Xb) {
        if (!h->have_pseudo)
            return GPE_ERR_STATE; // (the handle's M: the pseudo-inputs are replaced, not introduced)
        rc = gpe_sp_set_pseudo(h, Xb, h->M);
    }
    if (rc == GPE_OK)
        rc = gpe_sp_set_hparams(h, log_b, log_c, log_sig, jitter);
    if (rc == GPE_OK)
        rc = gpe_sp_compute(h);
    if (rc != GPE_OK)
        return rc;
    // the outputs are written together, after everything has succeeded
    std::vector<double> f((size_t)h->P), gx(d_xb ? (size_t)(h->M * h->D) : 0), gh((size_t)h->D + 2);
    rc = gpe_sp_nlml(h, f.data());
    if (rc == GPE_OK)
        rc = gpe_sp_grad(h, d_xb ? gx.data() : nullptr, gh.data());
    if (rc != GPE_OK)
        return rc;
    memcpy(nlml, f.data(), sizeof(double) * f.size());
    if (d_xb)
        memcpy(d_xb, gx.data(), sizeof(double) * gx.size());
    memcpy(d_hp, gh.data(), sizeof(double) * gh.size());
    return GPE_OK;
}

int gpe_sp_grad_phase_ms(gpe_sp_handle h, double* ms5)
{
    if (!h || !ms5)
        return GPE_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    for (int q = 0; q < 5; ++q)
        ms5[q] = h->gms[q];
    return GPE_OK;
}
