// select.hpp — greedy batch selection with hallucinated observations (include/gpe_batch_select.h): host side.  Kernels: select.hip.
// A part of engine.hip's translation unit (included there, once, behind query.hpp and joint.hpp, whose helpers it shares).
#pragma once

// Called with the handle's mutex held; M > 0, q > 0, arguments checked.
static int select_impl(gpe_ctx* c, const double* Xq, int64_t M, int q, int rule, double param, const double* mu_q, double var_add,
                       double obs_noise, int distinct, int64_t* idx, double* score, double* var_out, double* W, int64_t ldw)
{
    hipStream_t s = c->stream;
    digest_kernel(c);
    const int64_t N = c->N;
    PhaseDrain pd(c);
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device);
    const int64_t mc_max = round_up(M, 64);
    QtBufs b = served_layout(c, mc_max, N);
    const int64_t ldz = mc_max + 16; // as QtBufs::ldq of the transposed layout: even (16-byte rows), not a power of two
    const int nch = select_chunks(M, N, cus);
    const int64_t nrows = select_plan(M, N, cus, nullptr, 0);
    const size_t n_plan = 5 * (size_t)nrows;
    double *dZt2 = nullptr, *dZj = nullptr, *dWj = nullptr, *dPartV = nullptr, *dW = nullptr, *dMu = nullptr, *dPairs = nullptr, *dScore = nullptr;
    SelState* dState = nullptr;
    long long* dIdx = nullptr;
    int* dPicked = nullptr;
    int64_t* dPlan = nullptr;
    QueryScratch qs(c);
    if (const int e = qs.carve([&](Carver& cv) {
            qt_carve(b, cv);
            dZt2 = cv.take<double>(b.transposed ? 0 : (size_t)(ldz * N)); // Z with the points contiguous, where the layout has them not
            dZj = cv.take<double>((size_t)N);
            dWj = cv.take<double>((size_t)q);
            dPartV = cv.take<double>((size_t)nch * (size_t)ldz);
            dW = cv.take<double>((size_t)ldz * (size_t)q);
            dMu = cv.take<double>((size_t)mc_max);
            dPairs = cv.take<double>(2 * (size_t)select_fold_groups(M));
            dState = cv.take<SelState>(1); // (from here to the end of dPicked: cleared by one fill, below)
            dIdx = cv.take<long long>((size_t)q);
            dScore = cv.take<double>((size_t)q);
            dPicked = cv.take<int>((size_t)mc_max);
            dPlan = cv.take<int64_t>(n_plan);
        }))
        return e;

    std::vector<int64_t> plan(n_plan); // (alive until the stream has been waited for, below)
    (void)select_plan(M, N, cus, plan.data(), nrows);

    Marks mk(c->pool, s, c->prof);
    const int t0 = mk.mark();
    chunk_begin(c, b, true);
    chunk_head(c, b, Xq, true, M, true, mu_q == nullptr, nullptr, 0, M);
    ZView z = chunk_solve(c, b, M);
    chunk_var(c, b, M, z);
    if (z.kmajor) { // the rounds read Z with the points contiguous: transposed once
        launch_sel_transpose(s, z.p, z.ld, N, M, dZt2, ldz);
        z = ZView{dZt2, ldz, 0};
    }
    HIPCHK(c, hipMemsetAsync(dState, 0, (size_t)((char*)(dPicked + mc_max) - (char*)dState), s));
    HIPCHK(c, hipMemcpyAsync(dPlan, plan.data(), sizeof(int64_t) * n_plan, hipMemcpyHostToDevice, s));
    if (mu_q)
        HIPCHK(c, hipMemcpyAsync(dMu, mu_q, sizeof(double) * (size_t)M, hipMemcpyHostToDevice, s));
    const int t1 = mk.mark();
    SelRound g{};
    g.st = dState;
    g.plan = dPlan;
    g.nrows = nrows;
    g.nch = nch;
    g.Zt = z.p;
    g.ldz = z.ld;
    g.N = N;
    g.M = M;
    g.Qt = b.dQt;
    g.ldq = b.ldq;
    g.kp = &c->kp;
    g.zj = dZj;
    g.wj = dWj;
    g.part = dPartV;
    g.ldp = ldz;
    g.W = dW;
    g.ldw = ldz;
    g.var = b.dVar;
    g.mu = mu_q ? dMu : b.dKta; // (output 0: the first column of kta)
    g.picked = dPicked;
    g.pairs = dPairs;
    g.idx = dIdx;
    g.score = dScore;
    g.q = q;
    g.rule = rule;
    g.distinct = distinct;
    g.param = param;
    g.var_add = var_add;
    g.obs_noise = obs_noise;
    {
        // every round is enqueued now: the pick of a round is read from device memory by the next launch, no host wait between
        PhaseScope ps(c, GPE_PH_QUERY, 2.0 * (double)q * M * N);
        launch_sel_score0(s, g);
        for (int t = 0; t < q; ++t)
            launch_sel_round(s, g, t);
    }
    const int t2 = mk.mark();
    SelState st{};
    std::vector<long long> hidx((size_t)q);
    std::vector<double> hscore((size_t)q);
    HIPCHK(c, hipMemcpyAsync(&st, dState, sizeof(st), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(hidx.data(), dIdx, sizeof(long long) * (size_t)q, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(hscore.data(), dScore, sizeof(double) * (size_t)q, hipMemcpyDeviceToHost, s));
    if (var_out)
        HIPCHK(c, hipMemcpyAsync(var_out, b.dVar, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, s));
    if (const int e = stream_wait(c, "select_batch", true))
        return e;
    // rounds < fail - 1 are complete; round fail - 1 has its pick and score, not its column
    const int rounds = st.fail ? (int)st.fail : q, cols = st.fail ? (int)st.fail - 1 : q;
    for (int r = 0; r < rounds; ++r) {
        if (idx)
            idx[r] = (int64_t)hidx[(size_t)r];
        if (score)
            score[r] = hscore[(size_t)r];
    }
    if (W && cols > 0) {
        HIPCHK(c, copy2d_to_host(W, ldw, dW, ldz, M, cols, s));
        if (const int e = stream_wait(c, "select_batch", false))
            return e;
    }
    const int t3 = mk.mark();
    if (c->prof) {
        c->select_ms[0] = mk.ms(t0, t1);
        c->select_ms[1] = mk.ms(t1, t2);
        c->select_ms[2] = mk.ms(t2, t3);
    }
    return (int)st.fail;
}

int gpe_select_batch(gpe_handle c, const double* Xq, int64_t M, int q, int rule, double param, const double* mu_q, double var_add,
                     double obs_noise, int distinct, int64_t* idx, double* score, double* var_out, double* W, int64_t ldw)
{
    if (q < 0 || q > GPE_SELECT_MAX_ROUNDS || (rule != GPE_SELECT_UCB && rule != GPE_SELECT_EI && rule != GPE_SELECT_VAR))
        return GPE_ERR_ARG;
    if (!std::isfinite(param) || (rule == GPE_SELECT_UCB && param < 0.0) || !(obs_noise >= 0.0) || !std::isfinite(obs_noise))
        return GPE_ERR_ARG;
    const int e = joint_check(c, Xq, M, var_add); // (var_add: >= 0 and finite, as a jitter)
    if (e)
        return e;
    if ((distinct && q > M && M > 0) || (W && ldw < M))
        return GPE_ERR_ARG;
    if (M == 0 || q == 0)
        return GPE_OK;
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    return select_impl(c, Xq, M, q, rule, param, mu_q, var_add, obs_noise, distinct ? 1 : 0, idx, score, var_out, W, ldw);
}

int gpe_select_phase_ms(gpe_handle c, double* ms3) { return phase_ms_get(c, &gpe_ctx::select_ms, ms3); }

int gpe_debug_select_plan(int64_t M, int64_t N, int cus, int64_t* out, int64_t cap_rows) { return select_plan(M, N, cus, out, cap_rows); }
