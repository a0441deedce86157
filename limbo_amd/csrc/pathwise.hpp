// pathwise.hpp — posterior draws as functions of the query point (include/gpe_pathwise.h): host side.  Kernels: pathwise.hip.
// A part of engine.hip's translation unit (included there, once, behind qgrad.hpp, whose two triangular solves it shares).
#pragma once

// A path set: a snapshot of everything an evaluation reads, on a stream of its own — nothing of the handle is touched after
// gpe_paths_create, so whatever happens to the model later (more samples, another kernel, its destruction) cannot reach it.
struct gpe_paths_ctx {
    DEVBUF_LOCAL ~gpe_paths_ctx() = default;
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    int64_t N = 0, ldx = 0, ldr = 0;
    int D = 0, P = 0, R = 0, S = 0, ncols = 0;
    KParams kp;   // kp.D rows per point: the inputs and Lambda's projections
    LamParams lp;
    DevBuf<double> dXt;    // the samples, SoA with the projection rows, row r scaled by 1 / ell_r: kp.D x ldx
    DevBuf<double> dOm;    // Omega0, SoA: kp.D x ldr
    DevBuf<double> dPhase; // R
    DevBuf<double> dW;     // sqrt(2 sf2 / R) W: ldr x ncols
    DevBuf<double> dU;     // ldx x ncols
    DevBuf<double> dWork;  // an evaluation's chunk buffers, kept between calls
    int nsegF = 1, nsegK = 1;
    std::vector<hipEvent_t> pool; // the events of its phase timers (Marks): its own — an evaluation does not hold the handle's mutex
    double ms[4] = {0, 0, 0, 0};
};

// Segments of the basis functions (features or samples) per launch: enough workgroups for a handful of points (a lock-step search
// asks for q x starts of them), at least 128 basis functions each, no more partial sums than the column tiles leave room for.
// From the count and the columns alone — never from the batch.
static int paths_nseg(int64_t count, int ncols)
{
    const int64_t col_tiles = (ncols + 3) / 4;
    return (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)64, count / 128, 2048 / col_tiles}));
}
// points per chunk of an evaluation: the partial sums of a chunk stay under 2^25 doubles; a multiple of 64, from N, R, S P, D alone
static int64_t paths_chunk(const gpe_paths_ctx* ps)
{
    const int64_t per_point = (int64_t)ps->ncols * ((1 + ps->kp.D) * (int64_t)(ps->nsegF + ps->nsegK) + 1 + ps->D);
    return std::max<int64_t>(64, std::min<int64_t>(4096, (((int64_t)1 << 25) / per_point) / 64 * 64));
}
static bool all_finite(const double* a, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(a[i]))
            return false;
    return true;
}

#define PSCHK(ps, expr)                      \
    do {                                     \
        if ((expr) != hipSuccess)            \
            return GPE_ERR_HIP;              \
    } while (0)

// U for the draws [c0, c0 + nc): features at X, the residual (transposed, nc x N with leading dimension ldt, at dRt), then `solve`
// turns it into Wt = Rt K^-1 at the address it returns, and Wt^T goes into the set.  On the handle's stream, its mutex held.
static int paths_columns(gpe_ctx* c, gpe_paths_ctx* ps, const double* E, int c0, int nc, double* dRt, int64_t ldt, DevBuf<double>& tmp,
                         const std::function<const double*()>& solve)
{
    hipStream_t s = c->stream;
    const int64_t N = c->N;
    const int64_t pc_max = std::min<int64_t>(round_up(N, 64), 16384); // samples per feature launch
    const size_t n_part = (size_t)ps->nsegF * nc * pc_max, n_e = E ? (size_t)N * nc : 0;
    HIPCHK(c, tmp.reserve(n_part + n_e));
    double* dPart = tmp;
    double* dE = dPart + n_part;
    if (E)
        HIPCHK(c, hipMemcpyAsync(dE, E + (size_t)N * c0, sizeof(double) * n_e, hipMemcpyHostToDevice, s));
    Marks mk(ps->pool, s, true); // (the set is not shared yet)
    mk.mark();
    for (int64_t i0 = 0; i0 < N; i0 += pc_max) {
        const int64_t pc = std::min<int64_t>(pc_max, N - i0);
        PhaseScope sc(c, GPE_PH_QUERY, 2.0 * pc * ps->R * nc);
        launch_paths_basis(s, 0, false, c->dXt + i0, c->ld, pc, ps->dOm, ps->ldr, ps->R, ps->dPhase, ps->dW + (int64_t)c0 * ps->ldr, ps->ldr,
                           nc, ps->kp, ps->nsegF, dPart, pc_max);
        launch_paths_residual(s, dPart, ps->nsegF, pc_max, nc, pc, i0, c->dOm, c->ld, ps->S, c0, E ? dE : nullptr, N,
                              std::sqrt(c->noise + 1e-8), dRt, ldt);
    }
    mk.mark();
    const double* dWt = solve();
    launch_paths_untranspose(s, dWt, ldt, N, nc, ps->dU + (int64_t)c0 * ps->ldx, ps->ldx);
    mk.mark();
    if (const int e = stream_wait(c, "paths_create", true))
        return e;
    for (int q = 0; q < 2; ++q)
        ps->ms[q] += mk.ms(q, q + 1);
    return GPE_OK;
}

// The transposed layout: Rt in the place of the query's Kst, Wt = Rt L^-T L^-1 by the two solves of gpe_query_batch_grad
static int paths_solve_transposed(gpe_ctx* c, gpe_paths_ctx* ps, const double* E)
{
    const int64_t N = c->N;
    const int64_t mc_max = qt_rows_per_chunk(N, ps->ncols);
    QtBufs b = qt_layout(c, mc_max, N);
    QueryScratch qs(c);
    if (const int e = qs.carve(b))
        return e;
    qt_panels(c, b);
    DevBuf<double> tmp;
    int rc = GPE_OK;
    for (int c0 = 0; c0 < ps->ncols && rc == GPE_OK; c0 += (int)mc_max) {
        const int nc = (int)std::min<int64_t>(mc_max, ps->ncols - c0);
        rc = paths_columns(c, ps, E, c0, nc, b.dKst, b.ldq, tmp, [&]() -> const double* {
            qt_forward(c, b, nc);
            qt_backward(c, b, nc);
            return b.dKst;
        });
    }
    drain_phases(c);
    return rc;
}

// Where the transposed layout does not serve the model: Wt = Rt K^-1 in one product (K^-1: ensure_inv, as qgrad_impl)
static int paths_solve_by_inverse(gpe_ctx* c, gpe_paths_ctx* ps, const double* E)
{
    const int64_t N = c->N, ld = c->ld;
    {
        const int e = ensure_inv(c);
        if (e)
            return e;
    }
    const int64_t mc_max = nm_cols_per_chunk(ld, ps->ncols), ldt = mc_max + 16;
    DevBuf<double> mats, tmp;
    const size_t n_t = (size_t)(ldt * N), n_ki = (size_t)(ld * N);
    HIPCHK(c, mats.reserve(2 * n_t + n_ki));
    double* dRt = mats;
    double* dWt = dRt + n_t;
    double* dKi = dWt + n_t;
    kinv_operand(c, dKi);
    int rc = GPE_OK;
    for (int c0 = 0; c0 < ps->ncols && rc == GPE_OK; c0 += (int)mc_max) {
        const int nc = (int)std::min<int64_t>(mc_max, ps->ncols - c0);
        rc = paths_columns(c, ps, E, c0, nc, dRt, ldt, tmp, [&]() -> const double* {
            times_kinv(c, dKi, dRt, dWt, ldt, nc);
            return dWt;
        });
    }
    drain_phases(c);
    return rc;
}

static void paths_free(gpe_paths_ctx* ps)
{
    hipSetDevice(ps->device);
    if (ps->stream)
        hipStreamSynchronize(ps->stream);
    for (hipEvent_t e : ps->pool)
        hipEventDestroy(e);
    if (ps->stream)
        hipStreamDestroy(ps->stream);
    delete ps; // (the DevBufs free themselves)
}

int gpe_paths_create(gpe_handle c, int R, int S, const double* Omega0, const double* phase, const double* W, const double* E, gpe_paths* out)
{
    if (!c || !out || !Omega0 || !phase || !W || R < 1 || R > 16384 || S < 1)
        return GPE_ERR_ARG;
    *out = nullptr;
    if (!c->have_L || c->N <= 0)
        return GPE_ERR_STATE;
    if (c->host_K)
        return GPE_ERR_UNSUPPORTED;
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    if ((int64_t)S * c->P > 1024)
        return GPE_ERR_ARG;
    digest_kernel(c);
    const int64_t N = c->N;
    const int P = c->P, ncols = S * P, Rr = c->kp.D; // Rr = Dw: the rows of a point
    if (!all_finite(Omega0, (size_t)R * Rr) || !all_finite(phase, (size_t)R) || !all_finite(W, (size_t)R * ncols) ||
        (E && !all_finite(E, (size_t)N * ncols)))
        return GPE_ERR_ARG;

    gpe_paths_ctx* ps = new gpe_paths_ctx();
    struct Undo { // (every early return below frees the half-made set)
        gpe_paths_ctx* p;
        ~Undo()
        {
            if (p)
                paths_free(p);
        }
    } undo{ps};
    ps->device = c->device;
    ps->N = N, ps->D = c->D, ps->P = P, ps->R = R, ps->S = S, ps->ncols = ncols;
    ps->kp = c->kp;
    ps->lp = lam_params(c);
    ps->ldx = round_up(N, 16) + 16;
    ps->ldr = round_up(R, 16);
    ps->nsegF = paths_nseg(R, ncols);
    ps->nsegK = paths_nseg(N, ncols);
    HIPCHK(c, hipStreamCreateWithFlags(&ps->stream, hipStreamNonBlocking));
    HIPCHK(c, ps->dXt.reserve((size_t)(ps->ldx * Rr)));
    HIPCHK(c, ps->dOm.reserve((size_t)(ps->ldr * Rr)));
    HIPCHK(c, ps->dPhase.reserve((size_t)ps->ldr));
    HIPCHK(c, ps->dW.reserve((size_t)(ps->ldr * ncols)));
    HIPCHK(c, ps->dU.reserve((size_t)(ps->ldx * ncols)));

    hipStream_t s = c->stream;
    // host staging: Omega0 by rows, W with the features' amplitude (alive until the stream has been waited for, below)
    std::vector<double> om((size_t)ps->ldr * Rr, 0.0), w((size_t)ps->ldr * ncols, 0.0);
    for (int r = 0; r < R; ++r)
        for (int j = 0; j < Rr; ++j)
            om[(size_t)j * ps->ldr + r] = Omega0[(size_t)r * Rr + j];
    const double amp = std::sqrt(2.0 * c->kp.sf2 / R);
    for (int q = 0; q < ncols; ++q)
        for (int r = 0; r < R; ++r)
            w[(size_t)q * ps->ldr + r] = amp * W[(size_t)q * R + r];
    HIPCHK(c, hipMemcpyAsync(ps->dOm, om.data(), sizeof(double) * om.size(), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(ps->dW, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(ps->dPhase, 0, sizeof(double) * (size_t)ps->ldr, s));
    HIPCHK(c, hipMemcpyAsync(ps->dPhase, phase, sizeof(double) * (size_t)R, hipMemcpyHostToDevice, s));
    launch_paths_scale_rows(s, c->dXt, c->ld, ps->dXt, ps->ldx, N, ps->kp);

    const int rc = qt_enabled(c) ? paths_solve_transposed(c, ps, E) : paths_solve_by_inverse(c, ps, E);
    if (hipStreamSynchronize(s) != hipSuccess) // (the staging vectors, on every path)
        return GPE_ERR_HIP;
    if (rc)
        return rc;
    undo.p = nullptr;
    *out = ps;
    return GPE_OK;
}

// F / dF to the caller's arrays (either may be null), or — am != null — the running arg-max of every column
static int paths_eval_impl(gpe_paths_ctx* ps, const double* Xq, int64_t T, const double* mean_q, double* F, double* dF, int64_t* argmax,
                           double* fmax)
{
    if (!ps || T < 0 || (T > 0 && !Xq))
        return GPE_ERR_ARG;
    const bool want_am = argmax || fmax, grad = dF != nullptr;
    if (T == 0 || (!F && !dF && !want_am))
        return GPE_OK;
    const int D = ps->D, P = ps->P, Rr = ps->kp.D, ncols = ps->ncols;
    if (!all_finite(Xq, (size_t)T * D) || (mean_q && !all_finite(mean_q, (size_t)T * P)))
        return GPE_ERR_ARG;
    hipSetDevice(ps->device);
    std::lock_guard<std::mutex> lk(ps->mu);
    hipStream_t s = ps->stream;
    const int64_t N = ps->N, mc_max = std::min<int64_t>(paths_chunk(ps), round_up(T, 64)), ldq = mc_max;
    const int NS = paths_slots(grad, Rr);
    const size_t n_qrm = (size_t)(mc_max * D), n_qt = (size_t)(ldq * Rr), n_mq = mean_q ? (size_t)(mc_max * P) : 0;
    const size_t n_pf = (size_t)ps->nsegF * ncols * NS * (size_t)mc_max, n_pk = (size_t)ps->nsegK * ncols * NS * (size_t)mc_max;
    const size_t n_f = (size_t)mc_max * ncols, n_g = grad ? n_f * D : 0, n_am = 2 * (size_t)ncols;
    PSCHK(ps, ps->dWork.reserve(n_qrm + n_qt + n_mq + n_pf + n_pk + n_f + n_g + n_am));
    double* dQrm = ps->dWork;
    double* dQt = dQrm + n_qrm;
    double* dMq = dQt + n_qt;
    double* dPf = dMq + n_mq;
    double* dPk = dPf + n_pf;
    double* dFo = dPk + n_pk;
    double* dGo = dFo + n_f;
    double* dAm = dGo + n_g;
    ps->ms[2] = ps->ms[3] = 0.0;
    int rc = GPE_OK;
    for (int64_t t0 = 0; t0 < T && rc == GPE_OK; t0 += mc_max) {
        const int64_t mc = std::min<int64_t>(mc_max, T - t0);
        hipMemcpyAsync(dQrm, Xq + t0 * D, sizeof(double) * (size_t)(mc * D), hipMemcpyHostToDevice, s);
        if (mean_q)
            copy2d_from_host(dMq, mc_max, mean_q + t0, T, mc, P, s);
        launch_transpose_x(s, dQrm, mc, D, dQt, ldq, 0);
        if (ps->kp.k_lam > 0)
            launch_lambda_rows(s, dQt, ldq, 0, mc, ps->lp);
        Marks mk(ps->pool, s, true);
        mk.mark();
        launch_paths_basis(s, 0, grad, dQt, ldq, mc, ps->dOm, ps->ldr, ps->R, ps->dPhase, ps->dW, ps->ldr, ncols, ps->kp, ps->nsegF, dPf, mc_max);
        mk.mark();
        launch_paths_basis(s, 1, grad, dQt, ldq, mc, ps->dXt, ps->ldx, N, nullptr, ps->dU, ps->ldx, ncols, ps->kp, ps->nsegK, dPk, mc_max);
        launch_paths_fold(s, dPf, ps->nsegF, dPk, ps->nsegK, mc_max, NS, ncols, mc, ps->kp, ps->lp, mean_q ? dMq : nullptr, mc_max, ps->S,
                          (F || want_am) ? dFo : nullptr, mc_max, grad ? dGo : nullptr, mc_max);
        mk.mark();
        if (want_am)
            launch_paths_argmax(s, dFo, mc_max, mc, ncols, t0, t0 == 0, dAm);
        if (F)
            copy2d_to_host(F + t0, T, dFo, mc_max, mc, ncols, s);
        if (dF)
            copy2d_to_host(dF + t0, T, dGo, mc_max, mc, (int64_t)D * ncols, s);
        if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess)
            rc = GPE_ERR_HIP;
        else
            for (int q = 0; q < 2; ++q)
                ps->ms[2 + q] += mk.ms(q, q + 1);
    }
    if (rc == GPE_OK && want_am) {
        std::vector<double> am(n_am);
        PSCHK(ps, hipMemcpyAsync(am.data(), dAm, sizeof(double) * n_am, hipMemcpyDeviceToHost, s));
        PSCHK(ps, hipStreamSynchronize(s));
        for (int q = 0; q < ncols; ++q) {
            if (fmax)
                fmax[q] = am[2 * (size_t)q];
            if (argmax)
                memcpy(argmax + q, &am[2 * (size_t)q + 1], sizeof(int64_t));
        }
    }
    if (sizeof(double) * ps->dWork.capacity() > ((size_t)64 << 20)) // a large batch: give the memory back (as QueryScratch)
        ps->dWork.reset();
    return rc;
}

int gpe_paths_eval(gpe_paths ps, const double* Xq, int64_t T, const double* mean_q, double* F, double* dF)
{
    return paths_eval_impl(ps, Xq, T, mean_q, F, dF, nullptr, nullptr);
}

int gpe_paths_argmax(gpe_paths ps, const double* Xq, int64_t T, const double* mean_q, int64_t* argmax, double* fmax)
{
    return paths_eval_impl(ps, Xq, T, mean_q, nullptr, nullptr, argmax, fmax);
}

int gpe_paths_info(gpe_paths ps, int64_t* N, int* D, int* P, int* R, int* S)
{
    if (!ps)
        return GPE_ERR_ARG;
    if (N)
        *N = ps->N;
    if (D)
        *D = ps->D;
    if (P)
        *P = ps->P;
    if (R)
        *R = ps->R;
    if (S)
        *S = ps->S;
    return GPE_OK;
}

int gpe_paths_phase_ms(gpe_paths ps, double* ms4)
{
    if (!ps || !ms4)
        return GPE_ERR_ARG;
    std::lock_guard<std::mutex> lk(ps->mu);
    for (int q = 0; q < 4; ++q)
        ms4[q] = ps->ms[q];
    return GPE_OK;
}

int gpe_paths_destroy(gpe_paths ps)
{
    if (!ps)
        return GPE_ERR_ARG;
    paths_free(ps);
    return GPE_OK;
}
