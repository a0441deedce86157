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
// The helpers below are what every query-side call is built from (qgrad.hpp, pathwise.hpp, joint.hpp, select.hpp, kg.hpp, append.hpp,
// sparse.hpp, sparse_grad.hpp, included behind this file).  A new one is written against these and names no layout itself:
//   qt_enabled / qt_serves, qt_rows_per_chunk / nm_cols_per_chunk, qt_layout / nm_layout / served_layout   which layout, how many
//                                   points, its buffers
//   QueryScratch::carve(regions)    the call's lease of gpe_ctx::dQuery: the chunk buffers (qt_carve) and every region of the call's
//                                   own, each declared once with its type and count (Carver, carve.h)
//   PhaseDrain, Marks, stream_wait  the phase records drained on every way out, the call's own timer, the host's wait
//   chunk_begin(c, b, want_z)       once per call, in front of the first chunk whose Z is wanted
//   chunk_head(c, b, X, ...)        per chunk: points -> SoA -> cross kernel (-> kta)
//   chunk_solve(c, b, mc) -> ZView  Z = L^-1 Ks in the chunk's layout; the view says where it lies and how (z_operands: as the
//                                   operands of a matrix-core product over the samples, or over the points)
//   chunk_var(c, b, mc, z, ...)     var = k(v, v) - |z|^2 per point
// Below these, for what is particular to one layout: qt_panels, qt_forward (also against another context's factor), qt_backward
// (qgrad.hpp), kinv_operand / times_kinv, trsm_left_blocked.

// Which layout.  The transposed one serves a context whose outer panels are what the one-launch panel inverses take (inv.hip) and
// that has at least one of them; the marginal calls (query, gradients, path sets) also obey GPE_QUERY_T, read once per process.
// The joint posterior and the sparse model ask qt_serves alone; the blocked append goes point by point while it is false.
static bool qt_serves(const gpe_ctx* c) { return c->N >= NBO; }
static bool qt_enabled(const gpe_ctx* c)
{
    static const bool allowed = env_not_zero("GPE_QUERY_T");
    return allowed && qt_serves(c);
}
// Points per chunk: a chunk's matrices (points x N transposed, ld x points otherwise) stay under 2 GiB each, and no chunk is larger
// than the batch rounded up to 64.  From the model's size and M alone.
static const int64_t kChunkDoubles = (int64_t)1 << 28;
static int64_t qt_rows_per_chunk(int64_t N, int64_t M)
{
    return std::min<int64_t>(std::max<int64_t>(64, (kChunkDoubles / std::max<int64_t>(N, 1)) / 64 * 64), round_up(M, 64));
}
static int64_t nm_cols_per_chunk(int64_t ld, int64_t M)
{
    return round_up(std::min<int64_t>(std::max<int64_t>(64, kChunkDoubles / std::max<int64_t>(ld, 1)), round_up(M, 64)), 64);
}
// The tile of every product of a chunk is picked from N alone, never from the batch: the 128 x 128 and the 64 x 64 kernels round
// differently in the last bit (measured, round 6: a point's variance moved by 1.5e-15 with the size of the batch it was asked
// in, because launch_gemm_sub picks the tile from the live-tile count = from mc).  A point's answer must not depend on the
// batch around it (tests/test_gpu_configs.py: the 100 000-point batch of configs[2] bitwise equal to chunks of 4096).
static int qt_tile(int64_t N) { return N >= 1024 ? 128 : 64; }

// The buffers of one chunk of <= mc_max points, carved from gpe_ctx::dQuery, and the launches that fill them
struct QtBufs {
    bool transposed = true; // false: the N x M layout (nm_layout)
    int64_t mc_max = 0, ldq = 0, npan = 0, zcols = 0;
    int nseg = 1, qtile = 128;
    size_t n_qrm = 0, n_qt = 0, n_kst = 0, n_zt = 0, n_xp = 0, n_part = 0, n_kta = 0;
    double *dQrm = nullptr, *dQt = nullptr, *dKst = nullptr, *dZt = nullptr, *dXp = nullptr, *dPart = nullptr, *dKta = nullptr, *dVar = nullptr,
           *dKvv = nullptr;
};
// mc_max: points per chunk (a multiple of 64); zcols >= N: columns of Zt (the joint posterior pads its k range with zero columns)
// N_ (>= 0): size for that many samples instead of the handle's current count (the blocked append reserves for its last chunk)
static QtBufs qt_layout(const gpe_ctx* c, int64_t mc_max, int64_t zcols, int64_t N_ = -1)
{
    QtBufs b;
    const int64_t N = N_ >= 0 ? N_ : c->N, nbo = NBO;
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
    b.qtile = qt_tile(N);
    return b;
}
// b's regions, in the order they lie in the scratch (a region of the call's own list: QueryScratch::carve)
static void qt_carve(QtBufs& b, Carver& cv)
{
    b.dQrm = cv.take<double>(b.n_qrm);
    b.dQt = cv.take<double>(b.n_qt);
    b.dKst = cv.take<double>(b.n_kst); // the cross kernel, then the running right-hand side Acc
    b.dZt = cv.take<double>(b.n_zt);
    b.dXp = cv.take<double>(b.n_xp);
    b.dPart = cv.take<double>(b.n_part);
    b.dKta = cv.take<double>(b.n_kta);
    b.dVar = cv.take<double>((size_t)b.mc_max);
    b.dKvv = cv.take<double>((size_t)b.mc_max);
}
// The N x M layout in the same buffers — fewer samples than one outer panel,
// GPE_QUERY_T=0, caller-supplied cross kernels: Kst holds Ks (ld x mc_max, the samples contiguous) and is solved in place
// (trsm_left_blocked); no panel inverses, no partial sums; second: Zt is another matrix of that shape, else empty
static QtBufs nm_layout(const gpe_ctx* c, int64_t mc_max, bool second)
{
    QtBufs b = qt_layout(c, mc_max, c->N);
    b.transposed = false;
    b.ldq = mc_max;
    b.n_qt = (size_t)(b.ldq * std::max(xt_rows(c->D), 1));
    b.n_kst = (size_t)(c->ld * mc_max);
    b.n_zt = second ? b.n_kst : 0;
    b.n_xp = b.n_part = 0;
    return b;
}
// The layout that serves the model, GPE_QUERY_T not asked (the joint posterior, batch selection, the knowledge gradient, the sparse model)
static QtBufs served_layout(const gpe_ctx* c, int64_t mc_max, int64_t zcols, bool second = false)
{
    return qt_serves(c) ? qt_layout(c, mc_max, zcols) : nm_layout(c, mc_max, second);
}
extern "C++" {
namespace { // (file-local types with member functions: nothing of them is exported)
// gpe_ctx::dQuery for the length of one call: grown on request (contents are not kept) and, however the call ends, given back
// when a large batch has made it large — kept across calls while small, so that point queries do not malloc/free
struct QueryScratch {
    gpe_ctx* c;
    explicit QueryScratch(gpe_ctx* c_) : c(c_) {}
    QueryScratch(const QueryScratch&) = delete;
    ~QueryScratch() { release(); }
    void release() // (a call with more work behind its last chunk says so itself, early)
    {
        if (sizeof(double) * c->dQuery.capacity() > ((size_t)64 << 20))
            c->dQuery.reset();
    }
    // room for the regions the call lists (carve.h: counted, reserved, then placed — by the same list), from the scratch's start
    int carve(const std::function<void(Carver&)>& regions)
    {
        Carver count;
        regions(count);
        HIPCHK(c, c->dQuery.reserve(count.doubles()));
        Carver place(c->dQuery.get());
        regions(place);
        return GPE_OK;
    }
    int carve(QtBufs& b) // (a call with the chunk buffers alone)
    {
        return carve([&b](Carver& cv) { qt_carve(b, cv); });
    }
};

// The phase records of the call (PhaseScope: timed events in c->pending while profiling is on) added up and their events returned
// on every way out of it, an early return after a HIP error included.  Declared in front of the call's QueryScratch and Marks.
struct PhaseDrain {
    gpe_ctx* c;
    explicit PhaseDrain(gpe_ctx* c_) : c(c_) {}
    PhaseDrain(const PhaseDrain&) = delete;
    ~PhaseDrain() { drain_phases(c); }
};

// Where a chunk's Z = L^-1 Ks lies (chunk_solve): element (point m, sample i) at p[m + i ld] — or, kmajor, at p[m ld + i]: the
// samples, the k index of every product with Z, contiguous
struct ZView {
    const double* p = nullptr;
    int64_t ld = 0;
    int kmajor = 0;
    int64_t sm() const { return kmajor ? ld : 1; } // the strides of a point and of a sample
    int64_t si() const { return kmajor ? 1 : ld; }
};

// The call's own phases for the *_phase_ms exports: boundaries recorded on one stream with events of one pool (the handle's, under
// its mutex; a path set's own), and — after the caller's stream wait — the time between two of them.  Off: mark() records nothing
// and every interval is 0.  The events go back to the pool with the timer, on every way out of the call.
struct Marks {
    std::vector<hipEvent_t>& pool;
    hipStream_t s;
    bool on;
    std::vector<hipEvent_t> ev;
    Marks(std::vector<hipEvent_t>& pool_, hipStream_t s_, bool on_) : pool(pool_), s(s_), on(on_) {}
    Marks(const Marks&) = delete;
    ~Marks()
    {
        for (hipEvent_t e : ev)
            pool.push_back(e);
    }
    int mark() // the index of the boundary, -1 while off
    {
        if (!on)
            return -1;
        ev.push_back(get_event(pool));
        hipEventRecord(ev.back(), s);
        return (int)ev.size() - 1;
    }
    int count() const { return (int)ev.size(); }
    double ms(int i, int j) const
    {
        float t = 0.f;
        if (i >= 0 && j >= 0 && j < count() && hipEventSynchronize(ev[(size_t)j]) == hipSuccess)
            hipEventElapsedTime(&t, ev[(size_t)i], ev[(size_t)j]);
        return t;
    }
};

// What stands behind every gpe_*_phase_ms export: the handle's record of its last call of that kind, n values, under its mutex
template <int n> int phase_ms_get(gpe_ctx* c, double (gpe_ctx::*ms)[n], double* out)
{
    if (!c || !out)
        return GPE_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    std::copy(c->*ms, c->*ms + n, out);
    return GPE_OK;
}
} // namespace
} // extern "C++"

// The host waits for stream s; last_error: what a launch since the last wait left behind is consulted too (each call's own choice).
// On failure err = "<what>: stream sync failed" and GPE_ERR_HIP.
static int stream_wait(hipStream_t s, std::string& err, const char* what, bool last_error)
{
    if (hipStreamSynchronize(s) == hipSuccess && (!last_error || hipGetLastError() == hipSuccess))
        return GPE_OK;
    err = std::string(what) + ": stream sync failed";
    return GPE_ERR_HIP;
}
static int stream_wait(gpe_ctx* c, const char* what, bool last_error) { return stream_wait(c->stream, c->err, what, last_error); }

// Z views as the operands of C (-)= A B^T over the samples (k = N) — or, over_points, over the chunk's points (k = mc)
static void z_operands(GemmArgs& g, const ZView& a, const ZView& b, bool over_points = false)
{
    g.A = a.p;
    g.lda = a.ld;
    g.a_kmajor = over_points ? !a.kmajor : a.kmajor;
    g.B = b.p;
    g.ldb = b.ld;
    g.b_kmajor = over_points ? !b.kmajor : b.kmajor;
}

// X_p of every panel, compact (in front of the first chunk whose Zt is wanted)
static void qt_panels(gpe_ctx* c, const QtBufs& b)
{
    PhaseScope ps(c, GPE_PH_QUERY, 0.0);
    launch_inv_panels(c->stream, c->dA, c->ld, c->N, NBO, c->dXinv, b.dXp, 0, nullptr, 0);
}
// Dst = Src F^-T panel by panel (gp.hpp:620, transposed) for the mc rows of Src, on c's stream and in c's phases; F: the factor of
// context f — c itself, or another of c's device (the sparse model's Lm) — and X its compact panel inverses.  Src is destroyed.
static void qt_forward(gpe_ctx* c, const QtBufs& b, int64_t mc, const gpe_ctx* f, const double* X, double* Src, double* Dst)
{
    hipStream_t s = c->stream;
    const int64_t N = f->N, ld = f->ld, nbo = NBO, ldq = b.ldq;
    for (int64_t o0 = 0; o0 < N; o0 += nbo) {
        const int64_t pw = std::min<int64_t>(nbo, N - o0), oe = o0 + pw;
        {
            GemmArgs g{};
            g.C = Dst + o0 * ldq;
            g.ldc = ldq;
            g.A = Src + o0 * ldq;
            g.lda = ldq;
            g.B = X + (o0 / nbo) * (nbo * nbo);
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
            g.C = Src + oe * ldq;
            g.ldc = ldq;
            g.A = Dst + o0 * ldq;
            g.lda = ldq;
            g.B = f->dA + oe + o0 * ld;
            g.ldb = ld;
            g.m = mc;
            g.n = N - oe;
            g.k = pw;
            PhaseScope ps(c, GPE_PH_QUERY, gemm_flops(g));
            launch_gemm_sub(s, g);
        }
    }
}
// Zt = Kst L^-T against the model's own factor — Kst: a chunk's cross kernel, or right-hand sides a caller put in its place (pathwise.hpp)
static void qt_forward(gpe_ctx* c, const QtBufs& b, int64_t mc) { qt_forward(c, b, mc, c, b.dXp, b.dKst, b.dZt); }

// The head of one chunk of mc points in either layout: the points (row-major: on the host, copied to b.dQrm, or on the device
// already; null: none, a caller-supplied cross kernel is in b.dKst) -> SoA -> Lambda's rows (no launch for a kernel without
// Lambda); want_ks: the cross kernel in b's layout; want_kta: kta on the device and, kta != null, to kta[m0 + p M]
static void chunk_head(gpe_ctx* c, const QtBufs& b, const double* X, bool x_on_host, int64_t mc, bool want_ks, bool want_kta, double* kta,
                       int64_t m0, int64_t M)
{
    hipStream_t s = c->stream;
    const int64_t N = c->N, ld = c->ld, ldq = b.ldq;
    const int D = c->D, P = c->P;
    if (X && x_on_host) {
        hipMemcpyAsync(b.dQrm, X, sizeof(double) * (size_t)(mc * D), hipMemcpyHostToDevice, s);
        X = b.dQrm;
    }
    if (X) {
        launch_transpose_x(s, X, mc, D, b.dQt, ldq, 0);
        project_lambda(c, s, b.dQt, ldq, 0, mc);
    }
    if (want_ks) { // gp.hpp:626-632
        PhaseScope ps(c, GPE_PH_QUERY, 0.0);
        if (b.transposed) // k is symmetric: the cross kernel with the roles of samples and points exchanged IS the transposed block
            launch_build_Ks(s, b.dQt, ldq, mc, c->dXt, ld, N, c->kp, b.dKst, ldq);
        else
            launch_build_Ks(s, c->dXt, ld, N, b.dQt, ldq, mc, c->kp, b.dKst, ld);
    }
    if (!want_kta)
        return;
    PhaseScope ps(c, GPE_PH_QUERY, 2.0 * N * mc * P); // gp.hpp:615
    if (b.transposed)
        launch_kta_t(s, b.dKst, ldq, N, mc, c->dAl, ld, P, b.dKta, b.mc_max, b.dPart, ldq, b.nseg);
    else
        launch_kta(s, b.dKst, ld, N, mc, c->dAl, ld, P, b.dKta, b.mc_max);
    if (kta)
        for (int p = 0; p < P; ++p)
            hipMemcpyAsync(kta + m0 + (int64_t)p * M, b.dKta + (int64_t)p * b.mc_max, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s);
}
// Once per call, in front of the first chunk whose Z is wanted: what chunk_solve needs beside the factor
static void chunk_begin(gpe_ctx* c, const QtBufs& b, bool want_z)
{
    if (b.transposed && want_z)
        qt_panels(c, b);
}
// Z = L^-1 Ks for the mc points of the chunk whose cross kernel (or whatever a caller put in its place) is in b.dKst, which is
// destroyed (gp.hpp:620): by the panels into b.dZt, or by the blocked solve in place
static ZView chunk_solve(gpe_ctx* c, const QtBufs& b, int64_t mc)
{
    if (b.transposed) {
        qt_forward(c, b, mc);
        return ZView{b.dZt, b.ldq, 0};
    }
    trsm_left_blocked(c, c->dA, b.dKst, c->ld, c->N, mc, false, GPE_PH_QUERY);
    return ZView{b.dKst, c->ld, 1};
}
// var[m] = kvv[m] - sum_i z(m, i)^2 over c's N samples (gp.hpp:621), on c's stream.  kvv null: k(v_m, v_m) of the chunk's points,
// computed here into b.dKvv; else the caller's (zeros: minus the squared norm alone).  var null: b.dVar.
static void chunk_var(gpe_ctx* c, const QtBufs& b, int64_t mc, const ZView& z, const double* kvv = nullptr, double* var = nullptr)
{
    PhaseScope ps(c, GPE_PH_QUERY, 2.0 * c->N * mc);
    if (!kvv) {
        launch_kvv(c->stream, b.dQt, b.ldq, mc, c->kp, b.dKvv);
        kvv = b.dKvv;
    }
    if (!var)
        var = b.dVar;
    if (z.kmajor)
        launch_col_var(c->stream, z.p, z.ld, c->N, mc, kvv, var);
    else
        launch_row_var_t(c->stream, z.p, z.ld, c->N, mc, kvv, var, b.dPart, b.ldq, b.nseg);
}

// K^-1 as an operand where the transposed layout does not serve (gradients, path sets): a full symmetric copy at dKi (ld x N) of
// what ensure_inv left — its lower triangle — once per call, then per chunk Wt = Rt K^-1 (m x N, both ldt) as one product
static void kinv_operand(gpe_ctx* c, double* dKi)
{
    PhaseScope ps(c, GPE_PH_QUERY, 0.0);
    launch_copy2d(c->stream, c->dKinv, c->ld, dKi, c->ld, c->N, c->N);
    launch_symmetrize_from_lower(c->stream, dKi, c->ld, c->N);
}
static void times_kinv(gpe_ctx* c, const double* dKi, const double* dRt, double* dWt, int64_t ldt, int64_t m)
{
    GemmArgs g{};
    g.C = dWt;
    g.ldc = ldt;
    g.A = dRt;
    g.lda = ldt;
    g.B = dKi;
    g.ldb = c->ld;
    g.m = m;
    g.n = c->N;
    g.k = c->N;
    g.overwrite = 1;
    g.tile = qt_tile(c->N);
    PhaseScope ps(c, GPE_PH_QUERY, gemm_flops(g));
    launch_gemm_sub(c->stream, g);
}

// shared by gpe_query_batch (cross kernel built on the device from Xq) and gpe_query_batch_cross
// (cross kernel handed over by the caller): kta = Ks^T alpha, var = kvv - colsum((L^-1 Ks)^2)
static int query_impl(gpe_ctx* c, const double* Xq, const double* KsHost, int64_t M, double* kta, double* var)
{
    hipStream_t s = c->stream;
    digest_kernel(c);
    PhaseDrain pd(c);
    const int64_t N = c->N, ld = c->ld;
    const int D = c->D, P = c->P;
    if (c->small_path && Xq && N <= small_max_n() && M <= shell::SMALL_POINTS && (int64_t)M * D <= shell::SMALL_IN_DOUBLES && P <= GPE_MAX_P) {
        // the per-point query of an acquisition functor on a small GP: one launch (one workgroup per point), the
        // points read from and the results written to pinned host memory (small.hip)
        memcpy(c->shell.small_in(), Xq, sizeof(double) * (size_t)(M * D));
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
        q.xq_host = c->shell.small_in();
        q.kta_host = c->shell.small_kta();
        q.var_host = c->shell.small_var();
        q.seq = c->hSmallSeq;
        q.seq_val = ++c->small_seq;
        q.want_kta = kta ? 1 : 0;
        q.want_var = var ? 1 : 0;
        {
            PhaseScope ps(c, GPE_PH_QUERY, (double)N * N * M);
            launch_small_query(s, q, c->kp, lam_params(c));
        }
        ++c->small_calls;
        const int rc = small_wait(c, (int)M, q.seq_val);
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
    const bool few = sweep_ok && c->flow_solve && M <= GPE_MAX_P && (N + NB - 1) / NB <= 256;
    // the transposed layout for the device's own cross kernel; the N x M one for a caller's, for the sweep (its Z beside Ks) and
    // where the transposed one does not serve
    const bool transposed = Xq && !few && qt_enabled(c);
    const int64_t mc_max = few ? GPE_MAX_P : transposed ? qt_rows_per_chunk(N, M) : nm_cols_per_chunk(ld, M);
    QtBufs b = transposed ? qt_layout(c, mc_max, N) : nm_layout(c, mc_max, few);
    QueryScratch qs(c);
    if (const int e = qs.carve(b))
        return e;
    int rc = GPE_OK;
    chunk_begin(c, b, var != nullptr);
    for (int64_t m0 = 0; m0 < M && rc == GPE_OK; m0 += mc_max) {
        const int64_t mc = std::min<int64_t>(mc_max, M - m0);
        if (!Xq) // the caller's cross kernel in the place of the device's
            copy2d_from_host(b.dKst, ld, KsHost + m0 * N, N, N, mc, s);
        chunk_head(c, b, Xq ? Xq + m0 * D : nullptr, true, mc, Xq != nullptr, kta != nullptr, kta, m0, M);
        if (var) {
            ZView z;
            if (few) {
                PhaseScope ps(c, GPE_PH_QUERY, (double)N * N * mc);
                launch_trsv_fwd_flow(s, c->dA, ld, N, c->dXinv, b.dKst, ld, b.dZt, ld, (int)mc, c->dInfo + 1); // gp.hpp:620
                z = ZView{b.dZt, ld, 1};
            }
            else
                z = chunk_solve(c, b, mc);
            if (!Xq) // (a caller's cross kernel comes without the points: var is minus the squared norm alone)
                hipMemsetAsync(b.dKvv, 0, sizeof(double) * (size_t)mc, s);
            chunk_var(c, b, mc, z, Xq ? nullptr : b.dKvv);
            hipMemcpyAsync(var + m0, b.dVar, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s);
        }
        rc = stream_wait(c, "query_batch", false);
        if (rc == GPE_OK && few && var && flow_failed(c)) {
            // the one-launch sweep gave up (never expected): the same chunk through the blocked solve, in place
            chunk_var(c, b, mc, chunk_solve(c, b, mc), b.dKvv);
            hipMemcpyAsync(var + m0, b.dVar, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s);
            rc = stream_wait(c, "query_batch", false);
        }
    }
    return rc;
}
