"""Leave-one-out cross-validation on the device (gpe_log_loo_cv, gpe_log_loo_cv_grad, gpe_get_loo_weights) at N >= 896 and on
handles that are used again: every other LOO check of the suite runs at N <= 333, where the weight product W = K^-1 diag(c) K^-1
(csrc/inverse.hpp: loo_weights, ONE launch_gemm_sub call with m = n = k = N) only ever takes the register-staged 32 x 64 kernel,
K^-1 only its panel form below four panels, and K^-1 is never computed again after W was written into the U buffer of its recursion.

The checker is never the engine: tests/loo_ref.py (numpy / LAPACK, the literal form of gp.hpp:339-402), held against the C oracle
at a hundredth of the bars below by tests/test_loo_host.py.  Bars (tests/parity_checks.py, test_gpu_loo_cv_vs_oracle):
value 1e-9 relative; gradient 1e-6 in norm AND per component (tests/high_dim.py: grad_component_err); weights and K^-1 1e-8 in norm.

Routes (test_every_form_of_the_weight_product_is_reached reads them from the launch trace, in a run of its own; the trace names
the direct-to-LDS kernels, the two register-staged tile shapes share a name and are told apart by their grid, which
launch_tile's folded enumeration fixes per shape):
  N  896  k_gemm_glds64 (14 tile rows: 105 live 64 x 64 tiles)          K^-1: panel form, 4 panels, two-stream overlap
  N 1024  k_gemm_glds64                                                 K^-1: the smallest order of the recursion (inv2.hip)
  N 1100  k_gemm4 32 x 64 (1100 % 32 != 0, 171 live 64-tiles)           K^-1: ragged recursion; P = 11 in two GPE_MAX_P chunks
  N 2016  k_gemm_glds64, the last 64-tile half full (2016 = 63 x 32)
  N 2100  k_gemm4 64 x 64 (33 tile rows: 561 live tiles)
  N 2464  k_gemm_glds (128 x 128, 20 tile rows: 210 live tiles, ragged last tile, tri_tile_map)

Worst errors seen per check (MI355X, this file's output with -s; see each test for its cases):
  parity, six cases       value 1.9e-14   gradient 1.1e-13 in norm, 2.0e-12 per component   weights 1.9e-12   K^-1 8.5e-13
                          log-lik gradient 1.2e-13 in norm, 2.0e-13 per component
  reused handle           theta_2: K^-1 1.7e-12, LOO gradient 2.5e-14 / 6.0e-12, log-lik gradient 2.6e-14 / 2.2e-12; every answer
                          from theta_2 on bitwise a fresh handle's
  N grown in place        K^-1 1.7e-12, value 5.8e-15, gradient 2.7e-14 / 1.8e-13; against a fresh handle 3.7e-13 at the most
  update_alpha / clone    value 2.0e-14, gradient 5.7e-14 / 1.4e-13; bitwise
No case failed when these tests were written: every kernel form keeps its stores inside N x N, and K^-1's recursion reads nothing of
what W leaves below the diagonal (its leaves rewrite the diagonal blocks in full, its products read k >= i only).
"""
import re

import numpy as np
import pytest

from limbo_amd import _capi
from oracle import np_oracle as O
from tests import loo_ref as R
from tests.high_dim import grad_component_err
from tests.util import new_gp, relerr_norm

pytestmark = pytest.mark.gpu
BAR_VALUE, BAR_GRAD, BAR_W, BAR_KINV, BAR_LIK = 1e-9, 1e-6, 1e-8, 1e-8, 1e-10
BAR_FRESH = 1e-10  # a factor that was appended to against a full one: equal to rounding, not bitwise

#         N     D  P   kind        optimize_noise  form of the weight product
CASES = [(896, 3, 2, O.SE_ARD, True, "glds64"),
         (1024, 2, 1, O.MATERN32, False, "glds64"),
         (1100, 3, 11, O.SE_ARD, True, "tile32x64"),
         (2016, 2, 1, O.EXP, True, "glds64"),
         (2100, 2, 3, O.SE_ARD, False, "tile64x64"),
         (2464, 3, 2, O.MATERN52, True, "glds128")]
IDS = ["n%d" % c[0] for c in CASES]
FORMS = ("tile32x64", "tile64x64", "glds64", "glds128")


def value_err(got, ref):
    return abs(got - ref) / max(1.0, abs(ref))


def grad_errs(got, ref):
    assert got.shape == ref.shape
    return relerr_norm(got, ref), float(np.max(grad_component_err(got, ref)))


def check_grad(what, got, ref):
    e, ec = grad_errs(got, ref)
    print(f"    {what}: {e:.2e} in norm, {ec:.2e} per component")
    assert e < BAR_GRAD and ec < BAR_GRAD, (what, e, ec)


def check_norm(what, got, ref, bar):
    e = relerr_norm(got, ref)
    print(f"    {what}: {e:.2e}")
    assert e < bar, (what, e)


def check_value(what, got, ref, bar=BAR_VALUE):
    e = value_err(got, ref)
    print(f"    {what}: {e:.2e}  ({got!r})")
    assert e <= bar, (what, got, ref)


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


# ------------------------------------------------------------------------------------------------ a. parity per form
def parity_reference(N, D, P, kind, on):
    def build():
        X, Y, (th,) = R.make_problem(N, D, P, kind)
        om, _ = O.obs_mean_data(Y)
        return X, om, th, R.reference(kind, X, om, th, R.NOISE, on, want_W=True, want_lik_grad=True)

    return R.cached(("parity", N, D, P, kind, on), build)


@pytest.mark.parametrize("N,D,P,kind,on,form", CASES, ids=IDS)
def test_parity_at_the_sizes_that_reach_each_form(engine_lib, N, D, P, kind, on, form):
    """One handle: compute, log_loo_cv, log_loo_cv_grad, get_loo_weights, log_lik_grad, get_Kinv — the first three and K^-1 against
    tests/loo_ref.py, the log-likelihood gradient (which reads K^-1 after W went into the U buffer) against np_oracle.log_lik_grad;
    the gradient once more, bitwise.  Seen: value <= 1.9e-14 (N = 1100, P = 11), gradient <= 1.1e-13 in norm and <= 2.0e-12 per
    component (N = 2016, the exponential kernel), weights <= 1.9e-12, K^-1 <= 8.5e-13, log-lik gradient <= 2.0e-13."""
    X, om, th, ref = parity_reference(N, D, P, kind, on)
    print(f"\nN={N} D={D} P={P} kind={kind} noise={'on' if on else 'off'} ({form}):")
    h = new_gp(engine_lib, kind, X, om, th, R.NOISE)
    assert h.compute() == 0
    val = h.log_loo_cv()
    g = h.log_loo_cv_grad(on)
    W = h.get_loo_weights()
    gl = h.log_lik_grad(on)
    Kinv = h.get_Kinv()
    g2 = h.log_loo_cv_grad(on)
    h.close()
    check_value("LOO value", val, ref.value)
    check_grad("LOO gradient", g, ref.grad)
    check_norm("LOO weights", W, ref.W, BAR_W)
    check_grad("log-lik gradient", gl, ref.lik_grad)
    check_norm("K^-1", Kinv, ref.Kinv, BAR_KINV)
    assert np.array_equal(W, W.T)
    assert same(g, g2)


# ------------------------------------------------------------------------------------------------ route check
_TRACE_LINE = re.compile(r"^\s*\S+\s+\S+\s+\d+\s+(.+?)\s+grid=(\d+),(\d+),(\d+)\s+block=(\d+)\s*$")


def folded_grid(N, TM, TN):
    """Workgroups of launch_tile<TM, TN> (csrc/gemm.hip) for a lower-triangular N x N product: column tj folded with column
    tiles_n - 1 - tj, every super column as long as the longest."""
    tiles_m, tiles_n = -(-N // TM), -(-N // TN)

    def live(tj):
        need = tj * TN - (TM - 1)
        return tiles_m - min(tiles_m, 0 if need <= 0 else -(-need // TM))

    nsup = (tiles_n + 1) // 2
    fold = max(live(sc) + (live(tiles_n - 1 - sc) if tiles_n - 1 - sc != sc else 0) for sc in range(nsup))
    return nsup * max(fold, 1)


def classify(name, grid_x, N):
    if name.startswith("k_gemm_glds64"):
        return "glds64"
    if name.startswith("k_gemm_glds<"):
        return "glds128"
    if name.startswith("k_gemm4<"):
        g32, g64 = folded_grid(N, 32, 64), folded_grid(N, 64, 64)
        assert g32 != g64, (N, g32, g64)  # (otherwise the grid would not tell the two register-staged shapes apart)
        return {g32: "tile32x64", g64: "tile64x64"}.get(grid_x, "k_gemm4 with an unexpected grid %d" % grid_x)
    return name


@pytest.fixture(scope="module")
def routes(engine_lib, tmp_path_factory):
    """{N: form} of the weight product, from gpe_trace / gpe_trace_dump around ONE get_loo_weights call per N on a handle whose K^-1
    exists already (so that the traced launches are loo_weights' own); tracing is off again before any other test runs."""
    path = tmp_path_factory.mktemp("loo_trace") / "trace.txt"
    out = {}
    for N, D, P, kind, on, _ in CASES:
        X, Y, (th,) = R.make_problem(N, D, P, kind)
        om, _ = O.obs_mean_data(Y)
        h = new_gp(engine_lib, kind, X, om, th, R.NOISE)
        assert h.compute() == 0
        h.compute_inv_kernel()
        try:
            assert engine_lib.fn("trace")(1) == 0
            h.get_loo_weights()
            assert engine_lib.fn("trace_dump")(str(path).encode()) == 0
        finally:
            engine_lib.fn("trace")(0)
        h.close()
        recs = [m.groups() for m in map(_TRACE_LINE.match, path.read_text().splitlines()) if m]
        names = [r[0] for r in recs]
        assert "k_sym_colscale" in names, names
        i = names.index("k_sym_colscale")
        assert len(recs) == i + 2, names  # the scaled copy of K^-1, then the product: the last launch of loo_weights
        out[N] = classify(names[i + 1], int(recs[i + 1][1]), N)
        print(f"N={N}: {names[i + 1]} grid={recs[i + 1][1]} -> {out[N]}")
    return out


def test_every_form_of_the_weight_product_is_reached(routes):
    """A threshold of launch_gemm_sub_impl that moves fails here instead of silently dropping a form from the parity cases."""
    assert routes == {c[0]: c[5] for c in CASES}
    assert set(routes.values()) == set(FORMS)


# ------------------------------------------------------------------------------------------------ b. a reused handle
def reuse_problem(N, D, P, kind, on):
    def build():
        X, Y, ths = R.make_problem(N, D, P, kind, n_thetas=3)
        om, _ = O.obs_mean_data(Y)
        return X, om, ths, R.reference(kind, X, om, ths[1], R.NOISE, on, want_lik_grad=True)

    return R.cached(("reuse", N, D, P, kind, on), build)


@pytest.mark.parametrize("N,D,P,kind,on", [(1100, 3, 2, O.SE_ARD, True), (2016, 2, 1, O.MATERN52, True)], ids=["n1100", "n2016"])
def test_reused_handle_equals_a_fresh_one(engine_lib, N, D, P, kind, on):
    """What a LOO fit does in a loop.  On one handle: theta_1 compute, log_loo_cv_grad, get_loo_weights (W now lies in the U buffer
    of K^-1's recursion, whose pads were zero-filled once); hp_objective(theta_2) (K^-1 by the recursion over that buffer);
    get_Kinv, log_loo_cv, log_loo_cv_grad; theta_3 by set_kernel + compute, log_lik_grad, get_Kinv.  Every answer from theta_2 on is
    BITWISE what a fresh handle gives that is taken through the same calls for that theta only (the engine's results are run-to-run
    identical, hp_objective is 'bit for bit' the separate calls), and theta_2's K^-1 and gradients meet the bars.  This is where a
    store of W outside N x N, or a read by the recursion of what W left below the diagonal, would show.
    Seen: bitwise at both sizes; theta_2 K^-1 <= 1.7e-12, LOO gradient <= 6.0e-12 per component, log-lik gradient <= 2.2e-12."""
    X, om, (th1, th2, th3), ref = reuse_problem(N, D, P, kind, on)
    print(f"\nN={N} D={D} P={P} kind={kind}:")

    def at_theta2(h):
        lik, gl, rc = h.hp_objective(kind, th2, R.NOISE, optimize_noise=on, want_grad=True)
        assert rc == 0
        return dict(lik=lik, lik_grad=gl, Kinv=h.get_Kinv(), loo=h.log_loo_cv(), loo_grad=h.log_loo_cv_grad(on))

    def at_theta3(h):
        h.set_kernel(kind, th3, R.NOISE)
        assert h.compute() == 0
        return dict(lik_grad=h.log_lik_grad(on), Kinv=h.get_Kinv())

    used = new_gp(engine_lib, kind, X, om, th1, R.NOISE)
    assert used.compute() == 0
    used.log_loo_cv_grad(on)
    used.get_loo_weights()
    u2 = at_theta2(used)
    u3 = at_theta3(used)
    used.close()
    fresh = _capi.Handle(engine_lib)
    fresh.set_data(X, om)
    f2 = at_theta2(fresh)
    fresh.close()
    fresh = _capi.Handle(engine_lib)
    fresh.set_data(X, om)
    f3 = at_theta3(fresh)
    fresh.close()
    check_norm("theta_2 K^-1", u2["Kinv"], ref.Kinv, BAR_KINV)
    check_value("theta_2 LOO value", u2["loo"], ref.value)
    check_grad("theta_2 LOO gradient", u2["loo_grad"], ref.grad)
    check_value("theta_2 log-lik", u2["lik"], ref.lik, BAR_LIK)
    check_grad("theta_2 log-lik gradient", u2["lik_grad"], ref.lik_grad)
    for k in u2:
        print(f"    theta_2 {k}: used == fresh bitwise: {same(u2[k], f2[k])}")
    for k in u3:
        print(f"    theta_3 {k}: used == fresh bitwise: {same(u3[k], f3[k])}")
    for k in u2:
        assert same(u2[k], f2[k]), ("theta_2", k)
    for k in u3:
        assert same(u3[k], f3[k]), ("theta_3", k)


# ------------------------------------------------------------------------------------------------ c. N grows under a kept U buffer
GROW_D, GROW_P, GROW_KIND, GROW_ON = 3, 2, O.SE_ARD, True


def grow_problem(n_final):
    def build():
        X, Y, (th,) = R.make_problem(n_final, GROW_D, GROW_P, GROW_KIND)
        om, _ = O.obs_mean_data(Y)
        return X, Y, th, R.reference(GROW_KIND, X, om, th, R.NOISE, GROW_ON)

    return R.cached(("grow", n_final), build)


@pytest.mark.parametrize("sizes", [(1060, 1080), (1080, 1010, 1040)], ids=["pads_of_1060_at_1080", "1010_panel_form_to_1040_recursion"])
def test_samples_appended_under_a_kept_buffer(engine_lib, sizes):
    """set_data frees the U buffer, add_samples inside the capacity (1088) does not.  (1060, 1080): the recursion's pads were
    zero-filled at 1060 and W of 1060 written; at 1080 they are taken to be zero still.  (1080, 1010, 1040): capacity from a first
    set_data, K^-1 at 1010 in its panel form (whole tiles written, pads unknown) and W, then the recursion at 1040 on the same
    allocation.  After the append: log_loo_cv, log_loo_cv_grad, get_Kinv against the reference at the bars and against a fresh handle
    of the final N at 1e-10 relative (not bitwise: the appended factor differs from a full one in the last bits).
    Seen: K^-1 <= 1.7e-12, value <= 5.8e-15, gradient <= 1.8e-13 per component; against the fresh handle <= 3.7e-13 (K^-1)."""
    n1 = sizes[-1]
    X, Y, th, ref = grow_problem(n1)
    print(f"\nsizes {sizes}:")
    h = _capi.Handle(engine_lib)
    for n in sizes[:-1]:
        h.set_data(X[:n], O.obs_mean_data(Y[:n])[0])
    n0 = sizes[-2]
    h.set_kernel(GROW_KIND, th, R.NOISE)
    assert h.compute() == 0
    h.log_loo_cv_grad(GROW_ON)
    om1, _ = O.obs_mean_data(Y)
    assert h.add_samples(X[n0:n1], om1) == 0
    assert h.nb_samples() == n1
    got = (h.log_loo_cv(), h.log_loo_cv_grad(GROW_ON), h.get_Kinv())
    h.close()
    f = new_gp(engine_lib, GROW_KIND, X, om1, th, R.NOISE)
    assert f.compute() == 0
    fresh = (f.log_loo_cv(), f.log_loo_cv_grad(GROW_ON), f.get_Kinv())
    f.close()
    check_value("LOO value", got[0], ref.value)
    check_grad("LOO gradient", got[1], ref.grad)
    check_norm("K^-1", got[2], ref.Kinv, BAR_KINV)
    check_value("LOO value against the fresh handle", got[0], fresh[0], BAR_FRESH)
    check_norm("LOO gradient against the fresh handle", got[1], fresh[1], BAR_FRESH)
    e_c = float(np.max(grad_component_err(got[1], fresh[1])))
    print(f"    LOO gradient against the fresh handle, per component: {e_c:.2e}")
    assert e_c < BAR_FRESH
    check_norm("K^-1 against the fresh handle", got[2], fresh[2], BAR_FRESH)


# ------------------------------------------------------------------------------------------------ d. caches
CACHE_CASE = (1100, 3, 2, O.SE_ARD, True)


def cache_problem():
    def build():
        N, D, P, kind, on = CACHE_CASE
        X, Y, (th,) = R.make_problem(N, D, P, kind)
        om1, _ = O.obs_mean_data(Y)
        Y2 = np.stack([np.sin((p + 2) * X.sum(axis=1)) for p in range(P)], axis=1) + 0.1 * np.random.default_rng(N).normal(size=(N, P))
        om2, _ = O.obs_mean_data(Y2)
        return X, om1, om2, th, R.reference(kind, X, om2, th, R.NOISE, on)

    return R.cached(("cache",) + CACHE_CASE, build)


def test_update_alpha_keeps_inverse_and_loo_follows(engine_lib):
    """update_alpha(om_2) keeps K^-1 and gives a new alpha; the LOO value and gradient afterwards are those of om_2.  The handle that
    kept its K^-1 — and W of om_1 in the U buffer — against a handle that goes from compute(om_1) straight to update_alpha(om_2) and
    forms K^-1 only then: BITWISE (same factor, same sweep for alpha; what differs is the history of the buffers).  Against
    the reference: the bars.  Against a handle that was given om_2 from the start: 1e-10 relative — its alpha comes from the rows
    appended to the factorisation, not from update_alpha's sweep, so it is equal to rounding only.
    Seen: bitwise; value 2.0e-14, gradient 5.7e-14 / 1.4e-13; against the handle fitted to om_2 1.6e-15 and 5.7e-15, and indeed
    not bitwise."""
    N, D, P, kind, on = CACHE_CASE
    X, om1, om2, th, ref = cache_problem()
    print()
    kept = new_gp(engine_lib, kind, X, om1, th, R.NOISE)
    assert kept.compute() == 0
    kept.get_Kinv()
    kept.log_loo_cv_grad(on)
    kept.get_loo_weights()
    kept.update_alpha(om2)
    a = (kept.log_loo_cv(), kept.log_loo_cv_grad(on))
    kept.close()
    late = new_gp(engine_lib, kind, X, om1, th, R.NOISE)
    assert late.compute() == 0
    late.update_alpha(om2)
    b = (late.log_loo_cv(), late.log_loo_cv_grad(on))
    late.close()
    fit2 = new_gp(engine_lib, kind, X, om2, th, R.NOISE)
    assert fit2.compute() == 0
    c = (fit2.log_loo_cv(), fit2.log_loo_cv_grad(on))
    fit2.close()
    check_value("LOO value", a[0], ref.value)
    check_grad("LOO gradient", a[1], ref.grad)
    check_value("LOO value against the handle fitted to om_2", a[0], c[0], BAR_FRESH)
    check_norm("LOO gradient against the handle fitted to om_2", a[1], c[1], BAR_FRESH)
    print(f"    bitwise the handle fitted to om_2: value {a[0] == c[0]}, gradient {same(a[1], c[1])}")
    assert a[0] == b[0] and same(a[1], b[1])


def test_clone_without_u_buffer_gives_the_sources_loo(engine_lib):
    """A clone taken after get_Kinv and before any LOO call inherits K^-1 but has no U buffer (the branch at the top of loo_weights
    allocates one): its log_loo_cv_grad and get_loo_weights are the source's, bit for bit."""
    N, D, P, kind, on = CACHE_CASE
    X, om1, _, th, _ = cache_problem()
    h = new_gp(engine_lib, kind, X, om1, th, R.NOISE)
    assert h.compute() == 0
    h.get_Kinv()
    c = h.clone()
    gh, Wh = h.log_loo_cv_grad(on), h.get_loo_weights()
    gc, Wc = c.log_loo_cv_grad(on), c.get_loo_weights()
    h.close()
    c.close()
    assert np.all(np.isfinite(gh)) and np.linalg.norm(gh) > 0
    assert same(gh, gc)
    assert same(Wh, Wc)
