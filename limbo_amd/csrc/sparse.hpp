// sparse.hpp — the sparse pseudo-input GP (include/gpe_sparse.h; spgp.hpp:394-406, 491, 597-608): host side.  Kernels: sparse.hip.
// A part of engine.hip's translation unit (included there, once, behind query.hpp and joint.hpp, whose helpers it shares).
#pragma once

// One sparse model = two private dense contexts and the per-point vectors.
//   in : the pseudo-inputs as the samples of a dense SE-ARD model (P = 1, obs_mean = 0: alpha is never used); its compute is
//        L = chol(K(Xb, Xb) + jitter I) by the engine's schedule, a chunk of training rows (or of test points) is a batch of its
//        "query points": V^T is the Zt of the batched query.  Every launch of this file goes to ITS stream.
//   sc : "K is given" (as joint_scratch's): A is accumulated into its dKhost, r into its obs_mean; its compute leaves Lm, in the
//        right-hand-side rows under the factor bet^T = (Lm^-1 r)^T, and sum log diag(Lm) among the log-likelihood terms.
struct gpe_sp_ctx {
    DEVBUF_LOCAL ~gpe_sp_ctx() = default;
    int device = 0;
    gpe_ctx* in = nullptr;
    gpe_ctx* sc = nullptr;
    std::mutex mu;
    int64_t N = 0, M = 0, Mpad = 0;
    int D = 0, P = 0;
    bool have_data = false, have_pseudo = false, have_hp = false, computed = false, prof = false;
    std::vector<double> log_b;
    double log_c = 0, log_sig = 0, jitter = 0, c = 0, sig = 0;
    DevBuf<double> dX, dY, dEp; // N x D row-major, N x P (ld N), N
    DevBuf<double> dW, dPart, dBet, dXp2, dSums;
    DevBuf<int64_t> dPlan;
    std::vector<double> bet;  // M x P, host copy
    std::vector<double> nlml; // P
    double ms[5] = {0, 0, 0, 0, 0};
    DevBuf<double> dGrad; // the gradient's device block (sparse_grad.hpp)
    double gms[5] = {0, 0, 0, 0, 0};
    std::string err;
};

extern "C++" { // (this file is included inside engine.hip's extern "C" block: templates need C++ linkage)
namespace {

struct SpDevGuard {
    explicit SpDevGuard(gpe_sp_ctx* h) { hipSetDevice(h->device); }
};

int64_t sp_chunk(int64_t M, int64_t N)
{
    int64_t ch = sparse_default_chunk(M);
    if (const char* e = getenv("GPE_SPARSE_CHUNK")) { // read per call: tests force several chunks at small N
        const long long v = atoll(e);
        if (v > 0)
            ch = round_up((int64_t)v, 64);
    }
    return std::min<int64_t>(ch, round_up(N, 64));
}

// Which Gram path: GPE_SPARSE_GRAM=1 the split-k kernel (sparse.hip), =0 the composed one (a weighted copy of V through the general
// product), unset: the kernel while A has fewer lower 64 x 64 tiles than two per CU — where whole tiles leave the chip idle and the
// k split is what the kernel is for.  Measured (profiles/sparse_gp_timing.json, Gram phase at N = 1 048 576, kernel against
// composed): 13.9 / 49.1 ms at M = 512, 47.7 / 62.7 at M = 1024, and 181.8 / 153.8 at M = 2048, whose 528 tiles fill the chip
// un-split and where the general product's 128 x 128 tiles re-read V half as often.  Read per call.
bool sp_use_gram_kernel(int64_t M, int cus)
{
    if (const char* e = getenv("GPE_SPARSE_GRAM"))
        return atoi(e) != 0;
    const int64_t nt = (M + 63) / 64;
    return nt * (nt + 1) / 2 < 2 * (int64_t)cus;
}

// the layout of a chunk (query.hpp): the one that serves the inner model, with room for a second matrix beside Ks in either
QtBufs sp_layout(const gpe_ctx* c, int64_t mc_max) { return served_layout(c, mc_max, c->N, true); }

// the chunk's points (device, row-major mc x D) -> SoA, the cross kernel against the pseudo-inputs (spgp.hpp:396 / :597), V by the
// inner model's factor (:398 / :598) — a chunk of the batched query with the inner model as the model.  Its phases record nothing:
// the inner context's profiling is never on.  Returns V's place (needs chunk_begin).
ZView sp_v_chunk(gpe_sp_ctx* h, const QtBufs& b, const double* dXrm, int64_t mc)
{
    chunk_head(h->in, b, dXrm, false, mc, true, false, nullptr, 0, 0);
    return chunk_solve(h->in, b, mc);
}
// the chunk's other matrix (sp_layout): where V is not
double* sp_beside(const QtBufs& b, const ZView& z) { return z.p == b.dZt ? b.dKst : b.dZt; }

// (re)shape the scratch context for order M and P right-hand sides
int sp_scratch(gpe_sp_ctx* h)
{
    bool fresh = false;
    if (scratch_with_K(h->sc, h->M, h->P, &fresh) != GPE_OK) {
        h->err = "sparse GP: " + h->sc->err;
        return GPE_ERR_NOMEM;
    }
    return GPE_OK;
}

int sp_compute_locked(gpe_sp_ctx* h)
{
    h->computed = false;
    if (!h->have_data || !h->have_pseudo || !h->have_hp)
        return GPE_ERR_STATE;
    if (h->M > h->N)
        return GPE_ERR_ARG;
    gpe_ctx *in = h->in, *sc = h->sc;
    const int64_t N = h->N, M = h->M;
    const int D = h->D, P = h->P;
    // the inner model: theta = [log l_d = -1/2 log b_d .., log sigma_f = 1/2 log c], noise + 1e-8 = jitter (kernel.hpp:83)
    {
        double th[GPE_MAX_THETA];
        for (int d = 0; d < D; ++d)
            th[d] = -0.5 * h->log_b[(size_t)d];
        th[D] = 0.5 * h->log_c;
        int rc = gpe_set_kernel(in, GPE_KERNEL_SE_ARD, th, D + 1, h->jitter - 1e-8);
        if (rc == GPE_OK)
            rc = gpe_compute(in); // spgp.hpp:394-395
        if (rc < 0)
            h->err = "sparse GP: pseudo-input model: " + in->err;
        if (rc != GPE_OK)
            return rc;
    }
    {
        const int e = sp_scratch(h);
        if (e)
            return e;
    }
    std::lock_guard<std::mutex> lk(in->mu);
    hipStream_t s = in->stream;
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, in->device);
    const int64_t chunk = sp_chunk(M, N);
    const bool own_gram = sp_use_gram_kernel(M, cus);
    QtBufs b = sp_layout(in, chunk);
    QueryScratch qs(in);
    if (const int e = qs.carve(b)) {
        h->err = "sparse GP: " + in->err;
        return e;
    }
    const int64_t Mpad = h->Mpad, pstride = Mpad * Mpad;
    const int S0 = sparse_gram_slices(M, std::min(chunk, N), cus); // (the first chunk is the longest: no chunk has more slices)
    std::vector<int64_t> plan;
    if (own_gram) {
        const int64_t rows = sparse_gram_plan(M, N, chunk, cus, nullptr, 0);
        plan.resize((size_t)rows * 5);
        (void)sparse_gram_plan(M, N, chunk, cus, plan.data(), rows);
        HIPCHK(h, h->dPlan.reserve((size_t)(rows * 5)));
        if (S0 > 1)
            HIPCHK(h, h->dPart.reserve((size_t)(S0 * pstride)));
        HIPCHK(h, hipMemcpyAsync(h->dPlan, plan.data(), sizeof(int64_t) * plan.size(), hipMemcpyHostToDevice, s));
    }
    HIPCHK(h, h->dW.reserve((size_t)chunk));
    double* dA = sc->dKhost;
    const int64_t lda = sc->ld;
    HIPCHK(h, hipMemsetAsync(sc->dOm, 0, sizeof(double) * (size_t)(sc->ld * P), s)); // r
    if (!own_gram)
        launch_zero2d(s, dA, lda, Mpad, Mpad);
    chunk_begin(in, b, true);
    Marks mk(in->pool, s, h->prof); // per chunk three phases — V, ep and r, the Gram — of two boundaries each
    const int64_t nt = (M + 63) / 64, tiles = nt * (nt + 1) / 2;
    int64_t row0 = 0, slot0 = 0;
    for (int64_t n0 = 0; n0 < N; n0 += chunk) {
        const int64_t mc = std::min<int64_t>(chunk, N - n0);
        mk.mark();
        const ZView z = sp_v_chunk(h, b, h->dX + n0 * D, mc);
        const double* Z = z.p;
        const int64_t sn = z.sm(), si = z.si();
        mk.mark();
        mk.mark();
        launch_sp_ep(s, Z, sn, si, mc, M, h->c, h->sig, h->dEp + n0, h->dW);
        launch_sp_r(s, Z, sn, si, mc, M, h->dW, h->dY + n0, N, P, sc->dOm, sc->ld);
        mk.mark();
        mk.mark();
        if (own_gram) {
            const int S = sparse_gram_slices(M, mc, cus);
            const int64_t rows = tiles * S;
            if (S == 1)
                launch_sp_gram(s, Z, sn, si, h->dW, n0, M, h->dPlan + row0 * 5, rows, slot0, dA, lda, 0, n0 == 0 ? 1 : 2);
            else {
                launch_sp_gram(s, Z, sn, si, h->dW, n0, M, h->dPlan + row0 * 5, rows, slot0, h->dPart, Mpad, pstride, 0);
                launch_sp_fold(s, h->dPart, Mpad, pstride, S, n0 == 0 ? 1 : 0, M, dA, lda);
            }
            row0 += rows;
            slot0 += S;
        }
        else {
            // the composed path: a weighted copy of V, then the engine's general product on the k-contiguous operands
            double* Zw = sp_beside(b, z);
            launch_sp_scale(s, Z, sn, si, mc, M, h->dW, Zw);
            GemmArgs g{};
            g.C = dA;
            g.ldc = lda;
            z_operands(g, ZView{Zw, z.ld, z.kmajor}, z, true); // V^T diag(w) V: the k index is the chunk's points
            g.m = g.n = M;
            g.k = mc;
            g.tri = 1;
            g.overwrite = 2;
            launch_gemm_sub(s, g);
        }
        mk.mark();
    }
    launch_sp_diag_add(s, dA, lda, M, h->sig); // spgp.hpp:405: sig I + V V^T
    launch_symmetrize_from_lower(s, dA, lda, M);
    launch_sp_sums(s, h->dEp, N, h->dY, N, P, h->dSums);
    std::vector<double> sums((size_t)P + 1);
    HIPCHK(h, hipMemcpyAsync(sums.data(), h->dSums, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, s));
    if (const int e = stream_wait(s, h->err, "sparse GP", true))
        return e;
    if (h->prof)
        for (int ph = 0; ph < 3; ++ph) {
            h->ms[ph] = 0.0;
            for (int q = 2 * ph; q + 1 < mk.count(); q += 6)
                h->ms[ph] += mk.ms(q, q + 1);
        }
    qs.release();
    // Lm = chol(A) and bet = Lm^-1 r in the scratch context (A and r are complete: the stream has been waited for)
    int rc;
    {
        const auto t0 = std::chrono::steady_clock::now();
        rc = compute_enqueue(sc);
        if (rc == GPE_OK)
            rc = compute_finish(sc);
        if (rc < 0)
            h->err = "sparse GP: factorisation of A: " + sc->err;
        h->ms[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    if (rc > 0)
        return (int)(M + rc);
    if (rc < 0)
        return rc;
    const double sum_log_lm = sc->hScal[0];
    // bet^T sits in the right-hand-side rows under Lm; column form for the predictions, a host copy for the likelihood
    launch_rows_to_cols(sc->stream, sc->dA + M, sc->ld, M, P, h->dBet, Mpad);
    h->bet.assign((size_t)(M * P), 0.0);
    HIPCHK(h, copy2d_to_host(h->bet.data(), M, h->dBet, Mpad, M, P, sc->stream));
    HIPCHK(h, hipStreamSynchronize(sc->stream));
    h->nlml.assign((size_t)P, 0.0);
    for (int p = 0; p < P; ++p) { // spgp.hpp:491, with the real (n - m) / 2
        long double bb = 0.0L;
        for (int64_t i = 0; i < M; ++i)
            bb += (long double)h->bet[(size_t)(i + p * M)] * h->bet[(size_t)(i + p * M)];
        h->nlml[(size_t)p] = (double)((long double)sum_log_lm + 0.5L * (long double)(N - M) * (long double)h->log_sig
                                      + ((long double)sums[(size_t)p + 1] - bb) / (2.0L * (long double)h->sig) + 0.5L * (long double)sums[0]
                                      + 0.5L * (long double)N * std::log(2.0L * (long double)M_PI));
    }
    h->computed = true;
    return GPE_OK;
}

int sp_predict_locked(gpe_sp_ctx* h, const double* Xt, int64_t T, double* mu, double* s2)
{
    gpe_ctx *in = h->in, *sc = h->sc;
    std::lock_guard<std::mutex> lk(in->mu);
    hipStream_t s = in->stream;
    const int64_t M = h->M, Mpad = h->Mpad;
    const int D = h->D, P = h->P;
    // points per chunk: from M alone (a prediction must not depend on the batch around it)
    const int64_t mc_max = std::min<int64_t>(sparse_default_chunk(M), 16384);
    QtBufs b = sp_layout(in, mc_max);
    double *dV1 = nullptr, *dV2 = nullptr, *dZero = nullptr, *dS2 = nullptr, *dMu = nullptr, *dPartP = nullptr;
    QueryScratch qs(in);
    if (const int e = qs.carve([&](Carver& cv) {
            qt_carve(b, cv);
            dV1 = cv.take<double>((size_t)mc_max);
            dV2 = cv.take<double>((size_t)mc_max);
            dZero = cv.take<double>((size_t)mc_max);
            dS2 = cv.take<double>((size_t)mc_max);
            dMu = cv.take<double>((size_t)mc_max * P);
            dPartP = cv.take<double>((size_t)b.nseg * P * (size_t)b.ldq); // the partial sums of the P outputs
        })) {
        h->err = "sparse GP: " + in->err;
        return e;
    }
    Marks mk(in->pool, s, h->prof);
    mk.mark();
    HIPCHK(h, hipMemsetAsync(dZero, 0, sizeof(double) * (size_t)mc_max, s));
    chunk_begin(in, b, true);
    if (b.transposed) { // Lm's panel inverses beside L's, for the second solve
        const int64_t npan = (M + NBO - 1) / NBO;
        HIPCHK(h, h->dXp2.reserve((size_t)(npan * NBO * NBO)));
        launch_inv_panels(s, sc->dA, sc->ld, M, NBO, sc->dXinv, h->dXp2, 0, nullptr, 0);
    }
    int rc = GPE_OK;
    for (int64_t t0 = 0; t0 < T && rc == GPE_OK; t0 += mc_max) {
        const int64_t tc = std::min<int64_t>(mc_max, T - t0);
        HIPCHK(h, hipMemcpyAsync(b.dQrm, Xt + t0 * D, sizeof(double) * (size_t)(tc * D), hipMemcpyHostToDevice, s));
        const ZView z = sp_v_chunk(h, b, b.dQrm, tc); // lst (spgp.hpp:597-598)
        chunk_var(in, b, tc, z, nullptr, dV1);        // _k_diag (:630-634), c - |lst|^2
        // lmst = Lm^-1 lst (:599), into Kst, by the scratch context's factor; then - |lmst|^2 and the mean (:604)
        hipStream_t s2nd = s;
        if (!z.kmajor) {
            qt_forward(in, b, tc, sc, h->dXp2, b.dZt, b.dKst);
            chunk_var(in, b, tc, ZView{b.dKst, b.ldq, 0}, dZero, dV2);
            if (mu)
                launch_kta_t(s, b.dKst, b.ldq, M, tc, h->dBet, Mpad, P, dMu, mc_max, dPartP, b.ldq, b.nseg);
        }
        else {
            // the blocked solve launches on its context's stream: hand over to the scratch context's
            if (hipStreamSynchronize(s) != hipSuccess) {
                rc = GPE_ERR_HIP;
                break;
            }
            s2nd = sc->stream;
            trsm_left_blocked(sc, sc->dA, b.dKst, in->ld, M, tc, false, GPE_PH_QUERY);
            chunk_var(sc, b, tc, ZView{b.dKst, in->ld, 1}, dZero, dV2);
            if (mu)
                launch_kta(s2nd, b.dKst, in->ld, M, tc, h->dBet, Mpad, P, dMu, mc_max);
        }
        if (s2) {
            launch_sp_s2(s2nd, dV1, dV2, h->sig, tc, dS2); // :608
            HIPCHK(h, hipMemcpyAsync(s2 + t0, dS2, sizeof(double) * (size_t)tc, hipMemcpyDeviceToHost, s2nd));
        }
        if (mu)
            for (int p = 0; p < P; ++p)
                HIPCHK(h, hipMemcpyAsync(mu + t0 + (int64_t)p * T, dMu + (int64_t)p * mc_max, sizeof(double) * (size_t)tc, hipMemcpyDeviceToHost,
                                         s2nd));
        if (hipStreamSynchronize(s2nd) != hipSuccess || hipGetLastError() != hipSuccess)
            rc = GPE_ERR_HIP;
    }
    if (rc != GPE_OK)
        h->err = "sparse GP: predict: stream sync failed";
    mk.mark();
    if (h->prof)
        h->ms[4] = mk.ms(0, 1);
    return rc;
}

bool sp_finite(const double* v, int64_t n)
{
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i]))
            return false;
    return true;
}

} // namespace
} // extern "C++"

int gpe_sp_create(int device_id, gpe_sp_handle* out)
{
    if (!out)
        return GPE_ERR_ARG;
    gpe_sp_ctx* h = new gpe_sp_ctx();
    int rc = gpe_create(device_id, &h->in);
    if (rc == GPE_OK)
        rc = gpe_create(device_id, &h->sc);
    if (rc != GPE_OK) {
        if (h->in)
            gpe_destroy(h->in);
        delete h;
        return rc;
    }
    h->device = h->in->device;
    h->in->small_path = h->sc->small_path = false;
    *out = h;
    return GPE_OK;
}

int gpe_sp_destroy(gpe_sp_handle h)
{
    if (!h)
        return GPE_ERR_ARG;
    SpDevGuard g(h);
    hipStreamSynchronize(h->in->stream);
    hipStreamSynchronize(h->sc->stream);
    gpe_destroy(h->in);
    gpe_destroy(h->sc);
    delete h; // (frees the model's own buffers: both streams are idle)
    return GPE_OK;
}

const char* gpe_sp_last_error(gpe_sp_handle h) { return h ? h->err.c_str() : "null handle"; }

int gpe_sp_set_data(gpe_sp_handle h, const double* X, int64_t N, int D, const double* obs_zm, int P)
{
    if (!h || !X || !obs_zm || N < 1 || D < 1 || D > GPE_MAX_THETA - 2 || P < 1)
        return GPE_ERR_ARG;
    SpDevGuard g(h);
    std::lock_guard<std::mutex> lk(h->mu);
    h->computed = false;
    if (D != h->D)
        h->have_pseudo = h->have_hp = false; // (both are shaped by D)
    h->have_data = false;
    for (DevBuf<double>* b : {&h->dX, &h->dY, &h->dEp, &h->dSums}) // sized by the data exactly: a smaller set gives memory back
        b->reset();
    HIPCHK(h, h->dX.reserve((size_t)(N * D)));
    HIPCHK(h, h->dY.reserve((size_t)(N * P)));
    HIPCHK(h, h->dEp.reserve((size_t)N));
    HIPCHK(h, h->dSums.reserve((size_t)(P + 1)));
    HIPCHK(h, hipMemcpy(h->dX, X, sizeof(double) * (size_t)(N * D), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->dY, obs_zm, sizeof(double) * (size_t)(N * P), hipMemcpyHostToDevice));
    if (P != h->P)
        h->dBet.reset();
    h->N = N;
    h->D = D;
    h->P = P;
    h->have_data = true;
    return GPE_OK;
}

int gpe_sp_set_pseudo(gpe_sp_handle h, const double* Xb, int64_t M)
{
    if (!h || !Xb || M < 1 || M > 16384)
        return GPE_ERR_ARG;
    if (!h->have_data)
        return GPE_ERR_STATE;
    if (M > h->N || !sp_finite(Xb, M * h->D))
        return GPE_ERR_ARG;
    SpDevGuard g(h);
    std::lock_guard<std::mutex> lk(h->mu);
    h->computed = false;
    h->have_pseudo = false;
    std::vector<double> zero((size_t)M, 0.0);
    const int rc = gpe_set_data(h->in, Xb, M, h->D, zero.data(), 1);
    if (rc != GPE_OK) {
        h->err = "sparse GP: pseudo-input model: " + h->in->err;
        return rc;
    }
    h->dBet.reset();
    h->M = M;
    h->Mpad = round_up(M, 64);
    HIPCHK(h, h->dBet.reserve((size_t)(h->Mpad * h->P)));
    h->have_pseudo = true;
    return GPE_OK;
}

int gpe_sp_set_hparams(gpe_sp_handle h, const double* log_b, double log_c, double log_sig, double jitter)
{
    if (!h || !log_b)
        return GPE_ERR_ARG;
    if (!h->have_data)
        return GPE_ERR_STATE;
    if (!sp_finite(log_b, h->D) || !std::isfinite(log_c) || !std::isfinite(log_sig) || !std::isfinite(jitter) || !(jitter >= 1e-8))
        return GPE_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    h->computed = false;
    h->log_b.assign(log_b, log_b + h->D);
    h->log_c = log_c;
    h->log_sig = log_sig;
    h->jitter = jitter;
    h->c = std::exp(log_c);
    h->sig = std::exp(log_sig);
    h->have_hp = true;
    return GPE_OK;
}

int gpe_sp_compute(gpe_sp_handle h)
{
    if (!h)
        return GPE_ERR_ARG;
    SpDevGuard g(h);
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->have_data && h->have_pseudo && h->P > 0 && !h->dBet) // (set_data with another P after set_pseudo)
        HIPCHK(h, h->dBet.reserve((size_t)(h->Mpad * h->P)));
    return sp_compute_locked(h);
}

int gpe_sp_nlml(gpe_sp_handle h, double* out)
{
    if (!h || !out)
        return GPE_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->computed)
        return GPE_ERR_STATE;
    for (int p = 0; p < h->P; ++p)
        out[p] = h->nlml[(size_t)p];
    return GPE_OK;
}

int gpe_sp_objective(gpe_sp_handle h, const double* log_b, double log_c, double log_sig, double jitter, double* nlml)
{
    if (!h || !nlml)
        return GPE_ERR_ARG;
    int rc = gpe_sp_set_hparams(h, log_b, log_c, log_sig, jitter);
    if (rc == GPE_OK)
        rc = gpe_sp_compute(h);
    if (rc == GPE_OK)
        rc = gpe_sp_nlml(h, nlml);
    return rc;
}

int gpe_sp_predict(gpe_sp_handle h, const double* Xt, int64_t T, double* mu, double* s2)
{
    if (!h || T < 0 || (T > 0 && !Xt))
        return GPE_ERR_ARG;
    SpDevGuard g(h);
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->computed)
        return GPE_ERR_STATE;
    if (T == 0 || (!mu && !s2))
        return GPE_OK;
    return sp_predict_locked(h, Xt, T, mu, s2);
}

int gpe_sp_get_L(gpe_sp_handle h, double* L, int64_t ld)
{
    if (!h || !L)
        return GPE_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->computed)
        return GPE_ERR_STATE;
    return gpe_get_L(h->in, L, ld);
}

int gpe_sp_get_Lm(gpe_sp_handle h, double* Lm, int64_t ld)
{
    if (!h || !Lm)
        return GPE_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->computed)
        return GPE_ERR_STATE;
    return gpe_get_L(h->sc, Lm, ld);
}

int gpe_sp_get_bet(gpe_sp_handle h, double* bet)
{
    if (!h || !bet)
        return GPE_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->computed)
        return GPE_ERR_STATE;
    memcpy(bet, h->bet.data(), sizeof(double) * h->bet.size());
    return GPE_OK;
}

int gpe_sp_get_ep(gpe_sp_handle h, double* ep)
{
    if (!h || !ep)
        return GPE_ERR_ARG;
    SpDevGuard g(h);
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->computed)
        return GPE_ERR_STATE;
    HIPCHK(h, hipMemcpy(ep, h->dEp, sizeof(double) * (size_t)h->N, hipMemcpyDeviceToHost));
    return GPE_OK;
}

int gpe_sp_set_profiling(gpe_sp_handle h, int on)
{
    if (!h)
        return GPE_ERR_ARG;
    h->prof = on != 0;
    return GPE_OK;
}

int gpe_sp_phase_ms(gpe_sp_handle h, double* ms5)
{
    if (!h || !ms5)
        return GPE_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    for (int q = 0; q < 5; ++q)
        ms5[q] = h->ms[q];
    return GPE_OK;
}

int gpe_debug_gram_plan(int64_t M, int64_t N, int64_t chunk, int cus, int64_t* out, int64_t cap_rows)
{
    const int64_t rows = sparse_gram_plan(M, N, chunk, cus, out, cap_rows);
    return rows > INT32_MAX ? -1 : (int)rows;
}
