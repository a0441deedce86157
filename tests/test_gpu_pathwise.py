"""Pathwise posterior draws on the device (include/gpe_pathwise.h) and the C++ drop-in on top.

The checker is never the engine: tests/pathwise_ref.py (numpy / LAPACK; its two routes agree to 1e-11 or better on these inputs —
tests/test_pathwise_host.py — so the reference uses a thousandth of the bar at most).  Problems: query_grad_ref.make_problem, sigma_f = 1,
length scales 0.3 .. 1.0, noise 0.01.  The bar on F and dF: |got - ref| <= 1e-8 max(1, max|ref|), the project's bar for mu, sigma^2 and
their gradients."""
from pathlib import Path

import numpy as np
import pytest

from limbo_amd import _capi
from oracle import np_oracle as O
from tests import pathwise_ref as PR
from tests import query_grad_ref as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NOISE = R.NOISE
BAR = 1e-8
_cache = {}


def problem(kind, N, D, P, lam=0, seed=5):
    key = (kind, N, D, P, lam, seed)
    if key not in _cache:
        X, om = R.make_problem(N, D, P, seed)
        _cache[key] = dict(kind=kind, X=X, om=om, th=R.theta_of(kind, D, lam, seed), N=N, D=D, P=P, draws={}, refs={})
    return _cache[key]


def draws(pr, R_, S, seed=11):
    if (R_, S, seed) not in pr["draws"]:
        pr["draws"][(R_, S, seed)] = PR.make_draws(pr["kind"], pr["th"], pr["N"], pr["D"], pr["P"], R_, S, seed)
    return pr["draws"][(R_, S, seed)]


def reference(pr, R_, S, T, seed=6, with_E=True):
    """the points of a batch and their reference, computed once per (model, draws, batch) and left unchanged"""
    key = (R_, S, T, seed, with_E)
    if key not in pr["refs"]:
        Om, ph, W, E = draws(pr, R_, S)
        V = R.make_points(pr["X"], T, seed)
        pr["refs"][key] = (V, PR.reference(pr["kind"], pr["X"], pr["om"], pr["th"], NOISE, Om, ph, W, E if with_E else None, V))
    return pr["refs"][key]


def model(engine_lib, pr, n=None):
    h = _capi.Handle(engine_lib)
    h.set_data(pr["X"][:n], pr["om"][:n])
    h.set_kernel(pr["kind"], pr["th"], NOISE)
    assert h.compute() == 0
    return h


def check(got, ref, what=""):
    worst = {}
    for name, g, r in zip(("F", "dF"), got, ref):
        assert g.shape == r.shape, (name, g.shape, r.shape)
        worst[name] = float(np.max(np.abs(g - r))) / max(1.0, float(np.max(np.abs(r))))
    print(what, " ".join(f"{k}: {v:.3e}" for k, v in worst.items()))
    for name, v in worst.items():
        assert v <= BAR, (what, name, v)


def parity(engine_lib, pr, R_, S, T, what):
    V, ref = reference(pr, R_, S, T)
    h = model(engine_lib, pr)
    ps = h.paths(R_, S, *draws(pr, R_, S))
    check(ps.eval(V), ref, what)
    ps.close()
    h.close()


PARITY = {
    "se_ard_1100_d6": (O.SE_ARD, 1100, 6, 1, 0),
    "se_ard_700_d20": (O.SE_ARD, 700, 20, 1, 0),
    "se_ard_lambda2_600_d5": (O.SE_ARD, 600, 5, 1, 2),
    "matern52_520_d2": (O.MATERN52, 520, 2, 1, 0),
    "matern32_300_d3": (O.MATERN32, 300, 3, 1, 0),
    "exp_300_d3": (O.EXP, 300, 3, 1, 0),
    "se_ard_1100_d6_p2": (O.SE_ARD, 1100, 6, 2, 0),
}


@pytest.mark.parametrize("name", list(PARITY))
def test_parity_by_kind(engine_lib, name):
    parity(engine_lib, problem(*PARITY[name]), 1000, 8, 70, name)


@pytest.mark.parametrize("N", [200, 255, 256, 257, 1024, 1100])
def test_solve_edges(engine_lib, N):
    """U by the product with K^-1 below one outer panel, the first transposed sizes, the 64 / 128 tile switch at 1024"""
    parity(engine_lib, problem(O.SE_ARD, N, 6, 1), 1000, 8, 70, f"N={N}")


@pytest.mark.parametrize("S", [1, 3, 9, 65])
@pytest.mark.parametrize("R_", [1, 63, 64, 65, 1000])
def test_feature_tile_edges(engine_lib, R_, S):
    """one feature; 63, 64, 65 features (a segment of them is at least 128, so one segment with its tail); column tiles of 4, 8 and 16 not
    filled, and several of them"""
    parity(engine_lib, problem(O.SE_ARD, 300, 3, 1), R_, S, 70, f"R={R_} S={S}")


@pytest.mark.parametrize("D", [1, 20])
def test_low_and_high_dimension(engine_lib, D):
    """D = 20: two row tiles of 16 in the gradient pass"""
    parity(engine_lib, problem(O.SE_ARD, 300, D, 1), 1000, 8, 70, f"D={D}")


def test_batches_and_bits(engine_lib):
    """every batch holds training points verbatim and, from six points on, one point twice"""
    pr = problem(O.SE_ARD, 1100, 6, 1)
    h = model(engine_lib, pr)
    Om, ph, W, E = draws(pr, 1000, 8)
    ps = h.paths(1000, 8, Om, ph, W, E)
    for T in (1, 8, 9, 70, 700):
        V, ref = reference(pr, 1000, 8, T)
        got = ps.eval(V)
        check(got, ref, f"T={T}")
        if T >= 6:
            for g in got:
                assert np.array_equal(g[4], g[T - 1]), "the same point twice in a batch: the same bits"
    V700, _ = reference(pr, 1000, 8, 700)
    a, b = ps.eval(V700), ps.eval(V700)
    for x, y in zip(a, b):
        assert np.array_equal(x, y), "the call repeated gives the same bits"
    one = ps.eval(V700[333:334])
    sub = ps.eval(V700[300:370])
    for x, y, z in zip(one, sub, a):
        assert np.array_equal(x[0], z[333]), "a point asked alone and inside the 700: the same bits"
        assert np.array_equal(y, z[300:370])
    ps.close()
    # E = NULL is E = zeros
    p0, pz = h.paths(1000, 8, Om, ph, W, None), h.paths(1000, 8, Om, ph, W, np.zeros_like(E))
    V, ref = reference(pr, 1000, 8, 70, with_E=False)
    g0, gz = p0.eval(V), pz.eval(V)
    check(g0, ref, "E = NULL")
    for x, y in zip(g0, gz):
        assert np.array_equal(x, y), "E = NULL is bitwise E = zeros"
    p0.close()
    pz.close()
    h.close()


@pytest.mark.parametrize("D", [6, 20])
def test_partial_outputs(engine_lib, D):
    """F only and dF only are bitwise the full call's (the value-only pass and both gradient tilings)"""
    pr = problem(O.SE_ARD, 300 if D == 20 else 1100, D, 1)
    V, _ = reference(pr, 1000, 8, 70)
    h = model(engine_lib, pr)
    ps = h.paths(1000, 8, *draws(pr, 1000, 8))
    F, dF = ps.eval(V)
    F1, none = ps.eval(V, want=("F",))
    assert none is None and np.array_equal(F1, F)
    none, dF1 = ps.eval(V, want=("dF",))
    assert none is None and np.array_equal(dF1, dF)
    assert ps.eval(V, want=()) == (None, None)
    ps.close()
    h.close()


def test_mean_and_argmax(engine_lib):
    """argmax / fmax are np.argmax / max of the call's own F at T = 5000 (several chunks for these sizes), with a duplicated
    maximiser — the lowest index wins — and with a mean"""
    pr = problem(O.SE_ARD, 1100, 6, 2)
    h = model(engine_lib, pr)
    S, P, T = 8, 2, 5000
    ps = h.paths(1000, S, *draws(pr, 1000, S))
    rng = np.random.default_rng(77)
    V = rng.random((T, 6))
    mq = rng.standard_normal((T, P)) * 0.01
    F, _ = ps.eval(V, want=("F",), mean_q=mq)
    F0, _ = ps.eval(V, want=("F",))
    assert np.max(np.abs((F - F0) - mq[:, None, :])) <= 1e-14, "mean_q is added per output"
    # the maximiser of draw (0, 0) once more, behind the first: an exact tie
    first = int(np.argmax(F[:, 0, 0]))
    V[T - 3] = V[first]
    mq[T - 3] = mq[first]
    F, _ = ps.eval(V, want=("F",), mean_q=mq)
    assert F[T - 3, 0, 0] == F[first, 0, 0] and first < T - 3
    am, fm = ps.argmax(V, mean_q=mq)
    assert am.shape == (S, P) and fm.shape == (S, P)
    assert np.array_equal(am, np.argmax(F, axis=0)) and np.array_equal(fm, np.max(F, axis=0))
    assert am[0, 0] == first
    ps.close()
    h.close()


def test_snapshot(engine_lib):
    """the set answers the same bits after the handle has moved on; making and evaluating it does not change the handle's answers"""
    pr = problem(O.SE_ARD, 375, 6, 1)
    X, om = pr["X"], pr["om"]
    V = R.make_points(X, 70, 6)
    h = model(engine_lib, pr, 300)
    epoch0, ll0 = h.epoch(), h.log_lik()
    k0, v0 = h.query_batch(V)
    Om, ph, W, E = PR.make_draws(pr["kind"], pr["th"], 300, 6, 1, 1000, 8, 11)
    ps = h.paths(1000, 8, Om, ph, W, E)
    a = ps.eval(V)
    check(a, PR.reference(pr["kind"], X[:300], om[:300], pr["th"], NOISE, Om, ph, W, E, V), "N=300 of 375")
    assert h.epoch() == epoch0, "gpe_epoch does not move"
    assert h.log_lik() == ll0
    k1, v1 = h.query_batch(V)
    assert np.array_equal(k1, k0) and np.array_equal(v1, v0), "a later query_batch answers bitwise what it answered before"
    assert h.add_samples(X[300:375], om) == 0
    for x, y in zip(ps.eval(V), a):
        assert np.array_equal(x, y), "after add_samples"
    h.set_kernel(O.MATERN52, np.log([0.5, 1.3]), 0.02)
    assert h.compute() == 0
    for x, y in zip(ps.eval(V), a):
        assert np.array_equal(x, y), "after set_kernel + compute"
    h.close()
    for x, y in zip(ps.eval(V), a):
        assert np.array_equal(x, y), "after the handle's destruction"
    ps.close()


def test_one_real_size(engine_lib):
    pr = problem(O.SE_ARD, 4096, 6, 1)
    V, ref = reference(pr, 2048, 16, 2048)
    h = model(engine_lib, pr)
    ps = h.paths(2048, 16, *draws(pr, 2048, 16))
    check(ps.eval(V), ref, "N=4096 R=2048 S=16 T=2048")
    print(ps.phase_ms())
    ps.close()
    h.close()


def test_statuses(engine_lib):
    GPE_ERR_ARG, GPE_ERR_STATE, GPE_ERR_UNSUPPORTED = -1, -2, -5
    import ctypes as C
    create, ev, amx = engine_lib.fn("paths_create"), engine_lib.fn("paths_eval"), engine_lib.fn("paths_argmax")
    pr = problem(O.SE_ARD, 300, 3, 1)
    X, om = pr["X"], pr["om"]
    Rn, S = 64, 3
    Om, ph, W, E = PR.make_draws(pr["kind"], pr["th"], 300, 3, 1, Rn, S, 3)
    Wf, Ef = np.asfortranarray(W.reshape(Rn, S, order="F")), np.asfortranarray(E.reshape(300, S, order="F"))
    d = _capi._d
    out = C.c_void_p()

    def make(h, R_=Rn, S_=S, Om_=Om, ph_=ph, W_=Wf, E_=Ef, o=out):
        return create(h._h, R_, S_, d(Om_) if Om_ is not None else None, d(ph_) if ph_ is not None else None,
                      d(W_) if W_ is not None else None, d(E_) if E_ is not None else None, C.byref(o) if o is not None else None)

    h = _capi.Handle(engine_lib)
    h.set_data(X, om)
    h.set_kernel(O.SE_ARD, pr["th"], NOISE)
    assert make(h) == GPE_ERR_STATE, "before gpe_compute"
    assert h.compute() == 0
    live0 = _capi.debug_live_buffers(engine_lib)
    for kw in (dict(R_=0), dict(R_=16385), dict(S_=0), dict(S_=1025), dict(Om_=None), dict(ph_=None), dict(W_=None), dict(o=None)):
        assert make(h, **kw) == GPE_ERR_ARG, kw
    for name, arr in (("Om_", Om), ("ph_", ph), ("W_", Wf), ("E_", Ef)):
        for bad in (np.nan, np.inf):
            a = arr.copy(order="A")
            a.flat[a.size // 2] = bad
            assert make(h, **{name: a}) == GPE_ERR_ARG, (name, bad)
    assert _capi.debug_live_buffers(engine_lib) == live0, "a refused create leaves nothing behind"
    assert make(h) == 0 and out.value
    V = np.ascontiguousarray(X[:5] + 0.01)
    F, dF = np.zeros(5 * S), np.zeros(5 * 3 * S)
    am, fm = np.zeros(S, dtype=np.int64), np.zeros(S)
    amp = am.ctypes.data_as(C.POINTER(C.c_int64))
    assert ev(out, d(V), -1, None, d(F), d(dF)) == GPE_ERR_ARG
    assert ev(out, None, 5, None, d(F), d(dF)) == GPE_ERR_ARG
    assert ev(None, d(V), 5, None, d(F), d(dF)) == GPE_ERR_ARG
    assert ev(out, None, 0, None, d(F), d(dF)) == 0 and amx(out, None, 0, None, amp, d(fm)) == 0, "T = 0 returns 0 and does nothing"
    assert ev(out, d(V), 5, None, None, None) == 0
    assert not F.any() and not dF.any() and not fm.any()
    Vbad = V.copy()
    Vbad[2, 1] = np.nan
    assert ev(out, d(Vbad), 5, None, d(F), d(dF)) == GPE_ERR_ARG and amx(out, d(Vbad), 5, None, amp, d(fm)) == GPE_ERR_ARG
    mbad = np.full(5, np.inf)
    assert ev(out, d(V), 5, d(mbad), d(F), d(dF)) == GPE_ERR_ARG
    assert ev(out, d(V), 5, None, d(F), d(dF)) == 0 and F.any() and dF.any()
    assert amx(out, d(V), 5, None, amp, d(fm)) == 0 and fm[0] == F[:5].max() and am[0] == int(np.argmax(F[:5]))
    n, dd, p, r, s = C.c_int64(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert engine_lib.fn("paths_info")(out, C.byref(n), C.byref(dd), C.byref(p), C.byref(r), C.byref(s)) == 0
    assert (n.value, dd.value, p.value, r.value, s.value) == (300, 3, 1, Rn, S)
    ms = np.zeros(4)
    assert engine_lib.fn("paths_phase_ms")(out, d(ms)) == 0 and (ms >= 0).all()
    assert engine_lib.fn("paths_destroy")(out) == 0
    assert engine_lib.fn("paths_destroy")(None) == GPE_ERR_ARG
    h.close()
    # S P <= 1024 counts the outputs
    X2, om2 = R.make_problem(64, 2, 2, 1)
    h = _capi.Handle(engine_lib)
    h.set_data(X2, om2)
    h.set_kernel(O.SE_ARD, R.theta_of(O.SE_ARD, 2), NOISE)
    assert h.compute() == 0
    W2 = np.zeros((4, 513 * 2))
    assert create(h._h, 4, 513, d(np.zeros((4, 2))), d(np.zeros(4)), d(W2), None, C.byref(out)) == GPE_ERR_ARG
    h.close()
    # a handle whose kernel matrix came from the host has no device code for the kernel
    K = O.kernel_matrix(O.SE_ARD, X, pr["th"], NOISE)
    h = _capi.Handle(engine_lib)
    h.set_data(X, om)
    h.set_kernel(_capi.KERNEL_HOST_K, np.zeros(0), NOISE)
    h.set_K_host(K)
    assert h.compute() == 0
    assert make(h) == GPE_ERR_UNSUPPORTED
    h.close()


@pytest.mark.parametrize("N", [200, 1100])
def test_buffers(engine_lib, N):
    """gpe_debug_live_buffers returns to its value after close(), on both routes to U (K^-1 stays cached on the handle below one
    outer panel: the documented side effect, so the count is taken with it in place)"""
    pr = problem(O.SE_ARD, N, 6, 1)
    V, _ = reference(pr, 1000, 8, 70)
    h = model(engine_lib, pr)
    h.paths(1000, 8, *draws(pr, 1000, 8)).close()
    live0 = _capi.debug_live_buffers(engine_lib)
    ps = h.paths(1000, 8, *draws(pr, 1000, 8))
    ps.eval(V)
    ps.argmax(V)
    assert _capi.debug_live_buffers(engine_lib)[0] > live0[0]
    ps.close()
    assert _capi.debug_live_buffers(engine_lib) == live0
    h.close()


# ------------------------------------------------------------------------------------------------ the C++ drop-in on the device
from tests import test_pathwise_host as PH  # noqa: E402  (the driver's builder, protocol and numpy reference)
from tests import test_query_grad_host as H  # noqa: E402  (run_driver)


@pytest.mark.parametrize("kind", [O.SE_ARD, O.MATERN52], ids=["se_ard_600", "matern52_600"])
def test_cpp_dropin_on_the_device(tmp_path, kind):
    """sample_paths / eval / eval_grad / argmax of a device model (n = 600) against numpy, the prior's paths, the seeded overload"""
    drv = PH.build_driver("test_pathwise_dropin")
    c = PH.paths_case(kind, 600, 3, 2 if kind == O.SE_ARD else 1, 70, 256, 4, 80 + kind)
    out = H.run_driver(drv, "paths", PH.paths_case_text(c), tmp_path)
    assert out["host_resident"][0] == 0 and out["on_device"][0] == 1
    PH.check_paths(out, c, bar=BAR)


def test_cpp_thompson_paths_on_the_device(tmp_path):
    """thompson_paths_batch with q = 4 on a device model: each proposal in the box and on its own path at least that path's best
    candidate (the lock-step search returns the best point seen, and a point's value does not depend on its batch)"""
    drv = PH.build_driver("test_pathwise_dropin")
    out = H.run_driver(drv, "thompson", PH.thompson_case_text(600), tmp_path)
    assert out["host_resident"][0] == 0
    PH.check_thompson(out)
