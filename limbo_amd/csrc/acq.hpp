// acq.hpp — what the acquisition functions on a fitted model share on the host: the knowledge gradient (kg.hpp), the expected
// hypervolume improvement of two and of three objectives (ehvi.hpp, ehvi3.hpp), constrained expected improvement (cei.hpp), max-value entropy search (mes.hpp) and noisy
// expected improvement (nei.hpp).  A part of engine.hip's translation unit (included there, once, behind query.hpp, joint.hpp and
// select.hpp, whose helpers it builds on, and in front of the six).
//   cand_chunk_max, kValuesChunk      how many candidates go at once: through the model, and as beliefs handed over by the caller
//   cand_chunk                        a candidate chunk's head, solve and variance
//   cross_cov                         c = k(Xa, Xc) - Z_a^T Z_c of a resident point set with a candidate chunk
//   acq_batch(AcqCall, launch)        the fused call of an acquisition over marginal beliefs (ehvi, ehvi3, cei, mes)
//   acq_values(AcqValues, launch)     the same kernel on beliefs from the host
//   outs_ok                           output indices in [0, P), pairwise distinct
// An acquisition is a description and a function that launches its kernel for one chunk (AcqChunk): nothing here knows which.
#pragma once

static_assert(BELIEF_MAX == GPE_CEI_MAX_CONSTRAINTS + 1 && BELIEF_MAX >= GPE_MES_MAX_OUTPUTS, "BeliefArgs::col holds every caller's beliefs");

// Candidates per chunk of the N x M layout (fewer samples than one outer panel): the blocked solve picks its tile from the
// column count above some ten thousand columns, and a candidate's answer must not depend on the batch around it
static const int64_t kKgNmChunk = 8192;
// Beliefs (columns of slopes, conditional means) on the device at once where the caller hands them over: the *_values calls,
// gpe_kg_envelope; the cap of gpe_lognei_batch's chunk, whose U and cmean lie beside the chunk's own buffers
static const int64_t kValuesChunk = 16384;

// Candidates per chunk of a fused call: the chunk of a query in the layout that serves the model, from the model's size and M alone;
// cap: a bound of the caller's own beside it (NEI's; the default bounds nothing: no chunk has kChunkDoubles points)
static int64_t cand_chunk_max(const gpe_ctx* c, int64_t M, int64_t cap = kChunkDoubles)
{
    const int64_t N = c->N;
    return std::min<int64_t>(qt_serves(c) ? qt_rows_per_chunk(N, M) : std::min<int64_t>(nm_cols_per_chunk(c->ld, M), kKgNmChunk), cap);
}

// The head (want_kta: with k^T alpha of every output), solve and variance of a chunk of mc candidates, as a query's
static ZView cand_chunk(gpe_ctx* c, const QtBufs& b, const double* X, int64_t mc, bool want_kta)
{
    chunk_head(c, b, X, true, mc, true, want_kta, nullptr, 0, mc);
    const ZView z = chunk_solve(c, b, mc);
    chunk_var(c, b, mc, z);
    return z;
}

// dC (A x mc, ldc) = k(Xa, Xc) - Z_a^T Z_c on the matrix cores, for a resident set of A points (ba, za) and a candidate chunk (bc,
// zc): the tile from N alone, the k range whole (no split: nothing of the product depends on M or on where in the batch a
// candidate stands)
static void cross_cov(gpe_ctx* c, const QtBufs& ba, const ZView& za, int64_t A, const QtBufs& bc, const ZView& zc, int64_t mc, double* dC,
                      int64_t ldc)
{
    PhaseScope ps(c, GPE_PH_QUERY, 2.0 * (double)A * mc * c->N);
    launch_build_Ks(c->stream, ba.dQt, ba.ldq, A, bc.dQt, bc.ldq, mc, c->kp, dC, ldc);
    GemmArgs g{};
    g.C = dC;
    g.ldc = ldc;
    z_operands(g, za, zc);
    g.m = A;
    g.n = mc;
    g.k = c->N;
    g.tile = qt_tile(c->N);
    launch_gemm_sub(c->stream, g);
}

static bool outs_ok(const gpe_ctx* c, const int* outs, int n)
{
    for (int j = 0; j < n; ++j) {
        if (outs[j] < 0 || outs[j] >= c->P)
            return false;
        for (int i = 0; i < j; ++i)
            if (outs[i] == outs[j])
                return false;
    }
    return true;
}

// rows x cols doubles between a column-major host array and a device region (one column: the plain copy)
static hipError_t acq_copy(hipMemcpyKind kind, double* dst, int64_t ldd, const double* src, int64_t lds, int64_t rows, int cols, hipStream_t s)
{
    return cols == 1 ? hipMemcpyAsync(dst, src, sizeof(double) * (size_t)rows, kind, s) : copy2d(kind, dst, ldd, src, lds, rows, cols, s);
}

enum { ACQ_MAX_OUTS = 3 };
// One array an acquisition's kernel returns: cols columns per candidate, at the host column-major with leading dimension M (null:
// not asked for); on the device a region of cols x mc_max of its own, whether asked for or not
struct AcqOut {
    double* host;
    int cols;
};
// What the acquisition's launch function is handed for one chunk: the beliefs of mc candidates, complete; the constant input on
// the device; the region of each output, leading dimension ld
struct AcqChunk {
    hipStream_t s;
    BeliefArgs b;
    int64_t mc, ld;
    const double* konst;
    double* dev[ACQ_MAX_OUTS];
};
typedef std::function<void(const AcqChunk&)> AcqLaunch;

// The fused call over the marginal beliefs of nb outputs (indices outs) at M candidates: mean_add (M x nb, may be null) and var_add
// as the kernels take them; konst: n_konst doubles uploaded once in front of the loop; mu (M x nb) and var (M): the beliefs as
// used, null where not asked for; ms3: where the call's three phases go while profiling is on; what: the wait's name
struct AcqCall {
    const int* outs;
    int nb;
    const double* mean_add;
    double var_add;
    const double* konst;
    int64_t n_konst;
    AcqOut out[ACQ_MAX_OUTS];
    int n_out;
    double *mu, *var;
    double* ms3;
    const char* what;
};
// Called with the handle's mutex held; M > 0, arguments checked.
static int acq_batch(gpe_ctx* c, const double* Xc, int64_t M, const AcqCall& a, const AcqLaunch& launch)
{
    hipStream_t s = c->stream;
    digest_kernel(c);
    const int D = c->D;
    PhaseDrain pd(c);
    const int64_t mc_max = cand_chunk_max(c, M);
    QtBufs bc = served_layout(c, mc_max, c->N);
    AcqChunk ch{};
    double *dK = nullptr, *dAdd = nullptr, *dMu = nullptr;
    QueryScratch qs(c);
    if (const int e = qs.carve([&](Carver& cv) {
            qt_carve(bc, cv);
            dK = cv.take<double>((size_t)a.n_konst);
            dAdd = cv.take<double>((size_t)(a.nb * mc_max));
            for (int k = 0; k < a.n_out; ++k)
                ch.dev[k] = cv.take<double>((size_t)(a.out[k].cols * mc_max));
            dMu = cv.take<double>((size_t)(a.nb * mc_max));
        }))
        return e;
    if (a.n_konst > 0)
        HIPCHK(c, hipMemcpyAsync(dK, a.konst, sizeof(double) * (size_t)a.n_konst, hipMemcpyHostToDevice, s));
    ch.s = s;
    ch.ld = mc_max;
    ch.konst = dK;
    ch.b.mu = bc.dKta;
    ch.b.ldmu = bc.mc_max;
    ch.b.add = a.mean_add ? dAdd : nullptr;
    ch.b.lda = mc_max;
    ch.b.var = bc.dVar;
    ch.b.var_add = a.var_add;
    for (int j = 0; j < a.nb; ++j)
        ch.b.col[j] = a.outs[j];
    ch.b.mu_out = a.mu ? dMu : nullptr;
    ch.b.ldm = mc_max;

    Marks mk(c->pool, s, c->prof);
    double ms[3] = {0, 0, 0};
    chunk_begin(c, bc, true);
    int rc = GPE_OK;
    for (int64_t m0 = 0; m0 < M && rc == GPE_OK; m0 += mc_max) {
        const int64_t mc = ch.mc = std::min<int64_t>(mc_max, M - m0);
        const int u0 = mk.mark();
        cand_chunk(c, bc, Xc + m0 * D, mc, true);
        if (a.mean_add)
            HIPCHK(c, copy2d_from_host(dAdd, mc_max, a.mean_add + m0, M, mc, a.nb, s));
        const int u1 = mk.mark();
        {
            PhaseScope ps(c, GPE_PH_QUERY, 0.0);
            launch(ch);
        }
        const int u2 = mk.mark();
        for (int k = 0; k < a.n_out; ++k)
            if (a.out[k].host)
                HIPCHK(c, acq_copy(hipMemcpyDeviceToHost, a.out[k].host + m0, M, ch.dev[k], mc_max, mc, a.out[k].cols, s));
        if (a.mu)
            HIPCHK(c, copy2d_to_host(a.mu + m0, M, dMu, mc_max, mc, a.nb, s));
        if (a.var)
            HIPCHK(c, hipMemcpyAsync(a.var + m0, bc.dVar, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s));
        const int u3 = mk.mark();
        rc = stream_wait(c, a.what, true);
        ms[0] += mk.ms(u0, u1);
        ms[1] += mk.ms(u1, u2);
        ms[2] += mk.ms(u2, u3);
    }
    if (c->prof && rc == GPE_OK)
        for (int q = 0; q < 3; ++q)
            a.ms3[q] = ms[q];
    return rc;
}

// A piece of the beliefs a caller hands over: cols columns of means and of standard deviations (M x cols, leading dimension M;
// null: nothing to upload, the kernel does not read them), which become the beliefs col0 .. col0 + cols - 1
struct BeliefPiece {
    const double *mu, *sd;
    int col0, cols;
};
// The kernel alone on nb beliefs per candidate from the host, kValuesChunk candidates at a time: any handle, computed or not (its
// device, stream and scratch are all it takes).  konst, out, what: as AcqCall's.
struct AcqValues {
    int nb;
    BeliefPiece in[2];
    int n_in;
    const double* konst;
    int64_t n_konst;
    AcqOut out[ACQ_MAX_OUTS];
    int n_out;
    const char* what;
};
// M > 0, arguments checked; takes the handle's device and mutex itself.
static int acq_values(gpe_ctx* c, int64_t M, const AcqValues& a, const AcqLaunch& launch)
{
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t s = c->stream;
    const int64_t mc_max = std::min<int64_t>(M, kValuesChunk);
    AcqChunk ch{};
    double *dK = nullptr, *dMu = nullptr, *dSd = nullptr;
    QueryScratch qs(c);
    if (const int e = qs.carve([&](Carver& cv) {
            dK = cv.take<double>((size_t)a.n_konst);
            dMu = cv.take<double>((size_t)(a.nb * mc_max));
            dSd = cv.take<double>((size_t)(a.nb * mc_max));
            for (int k = 0; k < a.n_out; ++k)
                ch.dev[k] = cv.take<double>((size_t)(a.out[k].cols * mc_max));
        }))
        return e;
    if (a.n_konst > 0)
        HIPCHK(c, hipMemcpyAsync(dK, a.konst, sizeof(double) * (size_t)a.n_konst, hipMemcpyHostToDevice, s));
    ch.s = s;
    ch.ld = mc_max;
    ch.konst = dK;
    ch.b.mu = dMu;
    ch.b.sd = dSd;
    ch.b.ldmu = ch.b.lds = mc_max;
    for (int j = 0; j < a.nb; ++j)
        ch.b.col[j] = j;
    for (int64_t m0 = 0; m0 < M; m0 += mc_max) {
        const int64_t mc = ch.mc = std::min<int64_t>(mc_max, M - m0);
        for (int i = 0; i < a.n_in; ++i) {
            const BeliefPiece& p = a.in[i];
            if (p.cols > 0 && p.mu) {
                HIPCHK(c, acq_copy(hipMemcpyHostToDevice, dMu + p.col0 * mc_max, mc_max, p.mu + m0, M, mc, p.cols, s));
                HIPCHK(c, acq_copy(hipMemcpyHostToDevice, dSd + p.col0 * mc_max, mc_max, p.sd + m0, M, mc, p.cols, s));
            }
        }
        launch(ch);
        for (int k = 0; k < a.n_out; ++k)
            if (a.out[k].host)
                HIPCHK(c, acq_copy(hipMemcpyDeviceToHost, a.out[k].host + m0, M, ch.dev[k], mc_max, mc, a.out[k].cols, s));
        if (const int e = stream_wait(c, a.what, true))
            return e;
    }
    return GPE_OK;
}
