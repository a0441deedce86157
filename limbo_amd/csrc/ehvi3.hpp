// ehvi3.hpp — the three-objective expected hypervolume improvement over a Pareto front (include/gpe_ehvi3.h): host side — the
// front, the box tables, the two calls.  Kernel: ehvi3.hip.  A part of engine.hip's translation unit (included there, once, behind
// acq.hpp, whose two pipelines run it).
#pragma once

// The staircase of a sweep: points of the (a, b) plane none of which dominates another, ascending in a, hence descending in b; c:
// the coordinate the sweep descends in
struct Ehvi3Stair {
    struct Pt {
        double a, b, c;
    };
    std::vector<Pt> s;
    // does a point of the staircase dominate (a, b), or equal it?
    bool covers(double a, double b) const
    {
        const auto it = std::lower_bound(s.begin(), s.end(), a, [](const Pt& p, double v) { return p.a < v; });
        return it != s.end() && it->b >= b; // (the first point at or right of a is the highest of them)
    }
    // the points [lo, hi) that (a, b), itself not covered, dominates: those at or left of a that are not above b
    void dominated(double a, double b, size_t& lo, size_t& hi) const
    {
        hi = (size_t)(std::upper_bound(s.begin(), s.end(), a, [](double v, const Pt& p) { return v < p.a; }) - s.begin());
        lo = (size_t)(std::lower_bound(s.begin(), s.begin() + (ptrdiff_t)hi, b, [](const Pt& p, double v) { return p.b > v; }) - s.begin());
    }
    void replace(size_t lo, size_t hi, const Pt& q)
    {
        s.erase(s.begin() + (ptrdiff_t)lo, s.begin() + (ptrdiff_t)hi);
        s.insert(s.begin() + (ptrdiff_t)lo, q);
    }
};

int gpe_ehvi3_front(const double* F, int64_t n, const double* ref, double* out, int64_t* n_out)
{
    if (n < 0 || !ref || !n_out || (n > 0 && (!F || !out)) || !std::isfinite(ref[0]) || !std::isfinite(ref[1]) || !std::isfinite(ref[2]))
        return GPE_ERR_ARG;
    typedef std::array<double, 3> P3;
    std::vector<P3> p;
    p.reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const P3 f{F[3 * i], F[3 * i + 1], F[3 * i + 2]};
        if (f[0] != f[0] || f[1] != f[1] || f[2] != f[2])
            return GPE_ERR_ARG;
        if (std::isfinite(f[0]) && std::isfinite(f[1]) && std::isfinite(f[2]) && f[0] > ref[0] && f[1] > ref[1] && f[2] > ref[2])
            p.push_back(f);
    }
    // descending in (f3, f1, f2): whatever dominates or equals a point stands in front of it, so a point stays exactly when the
    // staircase of the points kept so far does not cover it in the (f1, f2) plane
    std::sort(p.begin(), p.end(), [](const P3& x, const P3& y) { return std::tie(x[2], x[0], x[1]) > std::tie(y[2], y[0], y[1]); });
    Ehvi3Stair st;
    std::vector<P3> keep;
    for (const P3& f : p) {
        if (st.covers(f[0], f[1]))
            continue;
        size_t lo, hi;
        st.dominated(f[0], f[1], lo, hi);
        st.replace(lo, hi, {f[0], f[1], f[2]});
        keep.push_back(f);
    }
    // descending in f3, ties ascending in f1, then in f2
    std::sort(keep.begin(), keep.end(), [](const P3& x, const P3& y) { return x[2] != y[2] ? x[2] > y[2] : std::tie(x[0], x[1]) < std::tie(y[0], y[1]); });
    for (size_t i = 0; i < keep.size(); ++i)
        for (int k = 0; k < 3; ++k)
            out[3 * i + k] = keep[i][(size_t)k];
    *n_out = (int64_t)keep.size();
    return GPE_OK;
}

// The table of height axis c of a front (row-major n x 3) appended to `rows` as {l_a, u_a, l_b, u_b, h}; false: the front is not
// prepared.  The sweep descends in f_c (stable: ties in the front's own order); a dominated or duplicate point shows as a point the
// staircase covers, or as one that removes a point of its own height.
static bool ehvi3_table(const double* front, int64_t n, const double* ref, int c, std::vector<double>& rows)
{
    if (n < 0 || n > GPE_EHVI3_MAX_FRONT || !ref || !std::isfinite(ref[0]) || !std::isfinite(ref[1]) || !std::isfinite(ref[2]) || (n > 0 && !front))
        return false;
    for (int64_t i = 0; i < n; ++i) {
        const double* f = front + 3 * i;
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(f[k]) || !(f[k] > ref[k]))
                return false;
        if (i > 0) { // descending in f3, ties ascending in f1, then in f2, strictly
            const double* g = f - 3;
            if (!(g[2] > f[2] || (g[2] == f[2] && (g[0] < f[0] || (g[0] == f[0] && g[1] < f[1])))))
                return false;
        }
    }
    const int a = c == 0 ? 1 : 0, b = c == 2 ? 1 : 2;
    std::vector<int64_t> ord((size_t)n);
    for (int64_t i = 0; i < n; ++i)
        ord[(size_t)i] = i;
    if (c != 2)
        std::stable_sort(ord.begin(), ord.end(), [&](int64_t i, int64_t j) { return front[3 * i + c] > front[3 * j + c]; });
    const double inf = std::numeric_limits<double>::infinity();
    auto row = [&](double la, double ua, double lb, double ub, double h) {
        if (la < ua && lb < ub)
            rows.insert(rows.end(), {la, ua, lb, ub, h});
    };
    Ehvi3Stair st;
    for (int64_t i : ord) {
        const Ehvi3Stair::Pt q{front[3 * i + a], front[3 * i + b], front[3 * i + c]};
        if (st.covers(q.a, q.b))
            return false;
        size_t lo, hi;
        st.dominated(q.a, q.b, lo, hi);
        for (size_t j = lo; j < hi; ++j)
            if (st.s[j].c == q.c)
                return false;
        // t + 1 strips from the left neighbour to q.a; under strip j the old staircase stands at the height of point lo + j, under
        // the last at the right neighbour's (r_b if there is none)
        double left = lo > 0 ? st.s[lo - 1].a : ref[a];
        for (size_t j = lo; j < hi; ++j) {
            row(left, st.s[j].a, st.s[j].b, q.b, q.c);
            left = st.s[j].a;
        }
        row(left, q.a, hi < st.s.size() ? st.s[hi].b : ref[b], q.b, q.c);
        st.replace(lo, hi, q);
    }
    // outside the final staircase: k + 1 unbounded strips of height r_c
    double left = ref[a];
    for (const Ehvi3Stair::Pt& p : st.s) {
        row(left, p.a, p.b, inf, ref[c]);
        left = p.a;
    }
    row(left, inf, ref[b], inf, ref[c]);
    return true;
}

int gpe_ehvi3_boxes(const double* front, int64_t n, const double* ref, int axis, double* boxes, int64_t cap, int64_t* n_boxes)
{
    std::vector<double> rows;
    if (axis < 0 || axis > 2 || !n_boxes || cap < 0 || (cap > 0 && !boxes) || !ehvi3_table(front, n, ref, axis, rows))
        return GPE_ERR_ARG;
    const int64_t k = (int64_t)rows.size() / 5;
    if (k > cap)
        return GPE_ERR_ARG;
    std::copy(rows.begin(), rows.end(), boxes);
    *n_boxes = k;
    return GPE_OK;
}

// The tables a call uploads: height axis 2 first (the value), then, with partials, axes 0 and 1; nb: their row counts
static bool ehvi3_tables(const double* front, int64_t n, const double* ref, bool want_partials, std::vector<double>& rows, int* nb)
{
    const int axes[3] = {2, 0, 1};
    for (int t = 0; t < (want_partials ? 3 : 1); ++t) {
        const size_t before = rows.size();
        if (!ehvi3_table(front, n, ref, axes[t], rows))
            return false;
        nb[t] = (int)((rows.size() - before) / 5);
    }
    return true;
}

// the box kernel for one chunk of either pipeline (acq.hpp); outputs: ehvi, partials
static void ehvi3_launch(const AcqChunk& ch, const int* nb, bool want_partials)
{
    Ehvi3Args q{};
    q.tables = ch.konst;
    q.ntab = want_partials ? 3 : 1;
    for (int t = 0; t < q.ntab; ++t)
        q.nb[t] = nb[t];
    q.b = ch.b;
    q.M = ch.mc;
    q.ehvi = ch.dev[0];
    q.partials = want_partials ? ch.dev[1] : nullptr;
    q.ldp = ch.ld;
    launch_ehvi3(ch.s, q);
}

// The box sums alone, on host-supplied beliefs: any handle, computed or not (its device, stream and scratch are all it takes)
int gpe_ehvi3_values(gpe_handle c, const double* front, int64_t n, const double* ref, const double* mu, const double* s, int64_t M, double* ehvi,
                     double* partials)
{
    std::vector<double> rows;
    std::array<int, 3> nb{0, 0, 0};
    if (M < 0 || !ehvi3_tables(front, n, ref, partials != nullptr, rows, nb.data()))
        return GPE_ERR_ARG;
    if (M == 0)
        return GPE_OK;
    if (!c || !mu || !s || !ehvi)
        return GPE_ERR_ARG;
    for (int64_t m = 0; m < 3 * M; ++m)
        if (s[m] < 0.0)
            return GPE_ERR_ARG;
    if (c->host_K)
        return GPE_ERR_UNSUPPORTED;
    // (beliefs, pieces and their count, constant input and its length, outputs and their count, the wait's name)
    const AcqValues a{3, {{mu, s, 0, 3}}, 1, rows.data(), (int64_t)rows.size(), {{ehvi, 1}, {partials, 6}}, 2, "ehvi3_values"};
    return acq_values(c, M, a, [=](const AcqChunk& ch) { ehvi3_launch(ch, nb.data(), partials != nullptr); });
}

int gpe_ehvi3_batch(gpe_handle c, const int* outs3, const double* Xc, int64_t M, const double* mean_add, double var_add, const double* front,
                    int64_t n, const double* ref, double* ehvi, double* partials, double* mu, double* var)
{
    std::vector<double> rows;
    std::array<int, 3> nb{0, 0, 0};
    if (!c || !outs3 || M < 0 || !(var_add >= 0.0) || !std::isfinite(var_add) || (M > 0 && !Xc)
        || !ehvi3_tables(front, n, ref, partials != nullptr, rows, nb.data()))
        return GPE_ERR_ARG;
    if (!c->have_L)
        return GPE_ERR_STATE;
    if (c->host_K)
        return GPE_ERR_UNSUPPORTED;
    if (!outs_ok(c, outs3, 3))
        return GPE_ERR_ARG;
    if (M == 0 || (!ehvi && !partials && !mu && !var))
        return GPE_OK;
    DevGuard g(c);
    std::lock_guard<std::mutex> lk(c->mu);
    // (belief columns and their count, mean_add, var_add, constant input and its length, outputs and their count, mu, var, phases, the wait's name)
    const AcqCall a{outs3, 3, mean_add, var_add, rows.data(), (int64_t)rows.size(), {{ehvi, 1}, {partials, 6}}, 2, mu, var, c->ehvi3_ms, "ehvi3_batch"};
    return acq_batch(c, Xc, M, a, [=](const AcqChunk& ch) { ehvi3_launch(ch, nb.data(), partials != nullptr); });
}

int gpe_ehvi3_phase_ms(gpe_handle h, double* ms3) { return phase_ms_get(h, &gpe_ctx::ehvi3_ms, ms3); }
