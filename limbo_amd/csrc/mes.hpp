// mes.hpp — max-value entropy search in the log domain (include/gpe_mes.h): host side.  Kernel: mes.hip.
// A part of engine.hip's translation unit (included there, once, behind acq.hpp, whose two pipelines run it).
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

// the kernel for one chunk of either pipeline (acq.hpp); the constant input: ystar; outputs: logmes, terms, partials
static void mes_launch(const AcqChunk& ch, int J, int K, bool want_terms, bool want_partials)
{
    MesArgs q{};
    q.J = J;
    q.K = K;
    q.ystar = ch.konst;
    q.b = ch.b;
    q.M = ch.mc;
    q.logmes = ch.dev[0];
    q.terms = want_terms ? ch.dev[1] : nullptr;
    q.partials = want_partials ? ch.dev[2] : nullptr;
    q.ldt = q.ldp = ch.ld;
    launch_mes(ch.s, q);
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
    // (beliefs, pieces and their count, constant input and its length, outputs and their count, the wait's name)
    const AcqValues a{J, {{mu, sd, 0, J}}, 1, ystar, (int64_t)J * K, {{logmes, 1}, {terms, J}, {partials, 2 * J}}, 3, "mes_values"};
    return acq_values(c, M, a, [=](const AcqChunk& ch) { mes_launch(ch, J, K, terms != nullptr, partials != nullptr); });
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
    if (!outs_ok(c, outs, J))
        return GPE_ERR_ARG;
    if (M == 0 || (!logmes && !terms && !partials && !mu && !var))
        return GPE_OK;
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    // (belief columns and their count, mean_add, var_add, constant input and its length, outputs and their count, mu, var, phases, the wait's name)
    const AcqCall a{outs, J, mean_add, var_add, ystar, (int64_t)J * K, {{logmes, 1}, {terms, J}, {partials, 2 * J}}, 3, mu, var, c->mes_ms, "mes_batch"};
    return acq_batch(c, Xc, M, a, [=](const AcqChunk& ch) { mes_launch(ch, J, K, terms != nullptr, partials != nullptr); });
}

int gpe_mes_phase_ms(gpe_handle c, double* ms3) { return phase_ms_get(c, &gpe_ctx::mes_ms, ms3); }
