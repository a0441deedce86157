// cei.hpp — constrained expected improvement in the log domain (include/gpe_cei.h): host side.  Kernel: cei.hip.
// A part of engine.hip's translation unit (included there, once, behind acq.hpp, whose two pipelines run it).
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
// the kernel for one chunk of either pipeline (acq.hpp); outputs: logcei, terms, partials
static void cei_launch(const AcqChunk& ch, int with_ei, double f_best, double xi, int C, const double* thr, bool want_terms, bool want_partials)
{
    CeiArgs q{};
    q.with_ei = with_ei ? 1 : 0;
    q.C = C;
    q.f_best = with_ei ? f_best : 0.0;
    q.xi = with_ei ? xi : 0.0;
    for (int k = 0; k < C; ++k)
        q.thr[k] = thr[k];
    q.b = ch.b;
    q.M = ch.mc;
    q.logcei = ch.dev[0];
    q.terms = want_terms ? ch.dev[1] : nullptr;
    q.partials = want_partials ? ch.dev[2] : nullptr;
    q.ldt = q.ldp = ch.ld;
    launch_logcei(ch.s, q);
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
    // (with_ei == 0: no objective belief is handed over, and none is read)
    // (beliefs, pieces and their count, constant input and its length, outputs and their count, the wait's name)
    const AcqValues a{1 + C, {{with_ei ? mu0 : nullptr, s0, 0, 1}, {mu_c, s_c, 1, C}}, 2, nullptr, 0,
                      {{logcei, 1}, {terms, 1 + C}, {partials, 2 + 2 * C}}, 3, "logcei_values"};
    return acq_values(c, M, a, [=](const AcqChunk& ch) { cei_launch(ch, with_ei, f_best, xi, C, thr, terms != nullptr, partials != nullptr); });
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
    int outs[1 + GPE_CEI_MAX_CONSTRAINTS] = {out0}; // the objective and the constraints together: in [0, P), pairwise distinct
    std::copy(con_outs, con_outs + C, outs + 1);
    if (!outs_ok(c, outs, 1 + C))
        return GPE_ERR_ARG;
    if (M == 0 || (!logcei && !terms && !partials && !mu && !var))
        return GPE_OK;
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    // (belief columns and their count, mean_add, var_add, constant input and its length, outputs and their count, mu, var, phases, the wait's name)
    const AcqCall a{outs, 1 + C, mean_add, var_add, nullptr, 0, {{logcei, 1}, {terms, 1 + C}, {partials, 2 + 2 * C}}, 3, mu, var, c->cei_ms, "logcei_batch"};
    return acq_batch(c, Xc, M, a, [=](const AcqChunk& ch) { cei_launch(ch, with_ei, f_best, xi, C, thr, terms != nullptr, partials != nullptr); });
}

int gpe_cei_phase_ms(gpe_handle c, double* ms3) { return phase_ms_get(c, &gpe_ctx::cei_ms, ms3); }
