// ehvi.hpp — the two-objective expected hypervolume improvement over a Pareto front (include/gpe_ehvi.h): host side.  Kernel: ehvi.hip.
// A part of engine.hip's translation unit (included there, once, behind acq.hpp, whose two pipelines run it).
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

// the strip kernel for one chunk of either pipeline (acq.hpp); outputs: ehvi, partials
static void ehvi_launch(const AcqChunk& ch, int64_t n, const double* ref, bool want_partials)
{
    EhviArgs q{};
    q.front = ch.konst;
    q.n = (int)n;
    q.r1 = ref[0];
    q.r2 = ref[1];
    q.b = ch.b;
    q.M = ch.mc;
    q.ehvi = ch.dev[0];
    q.partials = want_partials ? ch.dev[1] : nullptr;
    q.ldp = ch.ld;
    launch_ehvi2(ch.s, q);
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
    // (beliefs, pieces and their count, constant input and its length, outputs and their count, the wait's name)
    const AcqValues a{2, {{mu1, s1, 0, 1}, {mu2, s2, 1, 1}}, 2, front, 2 * n, {{ehvi, 1}, {partials, 4}}, 2, "ehvi2_values"};
    return acq_values(c, M, a, [=](const AcqChunk& ch) { ehvi_launch(ch, n, ref, partials != nullptr); });
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
    const int outs[2] = {out1, out2};
    if (!outs_ok(c, outs, 2))
        return GPE_ERR_ARG;
    if (M == 0 || (!ehvi && !partials && !mu && !var))
        return GPE_OK;
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    // (belief columns and their count, mean_add, var_add, constant input and its length, outputs and their count, mu, var, phases, the wait's name)
    const AcqCall a{outs, 2, mean_add, var_add, front, 2 * n, {{ehvi, 1}, {partials, 4}}, 2, mu, var, c->ehvi_ms, "ehvi2_batch"};
    return acq_batch(c, Xc, M, a, [=](const AcqChunk& ch) { ehvi_launch(ch, n, ref, partials != nullptr); });
}

int gpe_ehvi_phase_ms(gpe_handle c, double* ms3) { return phase_ms_get(c, &gpe_ctx::ehvi_ms, ms3); }
