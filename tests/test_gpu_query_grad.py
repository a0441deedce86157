"""The batched posterior with its gradient in the query point on the device (include/gpe_query_grad.h) and the C++ drop-in on top.

The checker is never the engine: tests/query_grad_ref.py (numpy / LAPACK; its two routes agree to 2.2e-12 or better on these
inputs — tests/test_query_grad_host.py — so the reference uses a ten-thousandth of the bar).  Inputs: X uniform in [0, 1]^D,
y = sin(3 X.u) + noise, sigma_f = 1, length scales 0.3 .. 1.0, noise 0.01.  The bar on all four outputs:
|got - ref| <= 1e-8 max(1, max|ref|)  (SURVEY §8c's bar for mu and sigma^2)."""
from pathlib import Path

import numpy as np
import pytest

from limbo_amd import _capi
from oracle import np_oracle as O
from tests import query_grad_ref as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NOISE = R.NOISE
BAR = 1e-8
NAMES = ("kta", "var", "dkta", "dvar")
_cache = {}


def problem(kind, N, D, P, lam=0, seed=5):
    key = (kind, N, D, P, lam, seed)
    if key not in _cache:
        X, om = R.make_problem(N, D, P, seed)
        _cache[key] = dict(kind=kind, X=X, om=om, th=R.theta_of(kind, D, lam, seed), refs={})
    return _cache[key]


def reference(pr, M, seed=6):
    """the points of a batch and their reference, computed once per (model, batch)"""
    if (M, seed) not in pr["refs"]:
        V = R.make_points(pr["X"], M, seed)
        pr["refs"][(M, seed)] = (V, R.reference(pr["kind"], pr["X"], pr["om"], pr["th"], NOISE, V))
    return pr["refs"][(M, seed)]


def model(engine_lib, pr, n=None):
    h = _capi.Handle(engine_lib)
    h.set_data(pr["X"][:n], pr["om"][:n])
    h.set_kernel(pr["kind"], pr["th"], NOISE)
    assert h.compute() == 0
    return h


def check(got, ref, what=""):
    worst = {}
    for name, g, r in zip(NAMES, got, ref):
        assert g.shape == r.shape, (name, g.shape, r.shape)
        worst[name] = float(np.max(np.abs(g - r))) / max(1.0, float(np.max(np.abs(r))))
    print(what, " ".join(f"{k}: {v:.3e}" for k, v in worst.items()))
    for name, v in worst.items():
        assert v <= BAR, (what, name, v)
    return worst


PARITY = {
    "se_ard_300_d3": (O.SE_ARD, 300, 3, 1, 0),
    "se_ard_1100_d6_p2": (O.SE_ARD, 1100, 6, 2, 0),
    "se_ard_700_d20": (O.SE_ARD, 700, 20, 1, 0),
    "se_ard_lambda2_600_d5": (O.SE_ARD, 600, 5, 1, 2),
    "matern52_520_d2": (O.MATERN52, 520, 2, 1, 0),
    "matern32_300_d3": (O.MATERN32, 300, 3, 1, 0),
    "exp_300_d3": (O.EXP, 300, 3, 1, 0),
}


@pytest.mark.parametrize("name", list(PARITY))
def test_parity_by_kind(engine_lib, name):
    pr = problem(*PARITY[name])
    V, ref = reference(pr, 70)
    h = model(engine_lib, pr)
    check(h.query_batch_grad(V), ref, name)
    h.close()


@pytest.mark.parametrize("N", [200, 255, 256, 257, 1024, 1100])
def test_panel_and_tile_edges(engine_lib, N):
    """the K^-1 path below one outer panel, the first transposed sizes, the 64 / 128 tile switch at 1024"""
    pr = problem(O.SE_ARD, N, 6, 1)
    V, ref = reference(pr, 70)
    h = model(engine_lib, pr)
    check(h.query_batch_grad(V), ref, f"N={N}")
    h.close()


@pytest.mark.parametrize("N", [200, 1100])
def test_batch_sizes(engine_lib, N):
    """every batch holds training points verbatim (z = 0) and, from six points on, one point twice"""
    pr = problem(O.SE_ARD, N, 6, 2)
    h = model(engine_lib, pr)
    for M in (1, 8, 9, 70, 700):
        V, ref = reference(pr, M)
        got = h.query_batch_grad(V)
        check(got, ref, f"N={N} M={M}")
        if M >= 6:
            for g in got:
                assert np.array_equal(g[4], g[M - 1]), "the same point twice in a batch: the same bits"
    h.close()


def test_one_real_size(engine_lib):
    pr = problem(O.SE_ARD, 4096, 6, 1)
    V, ref = reference(pr, 2048)
    h = model(engine_lib, pr)
    check(h.query_batch_grad(V), ref, "N=4096 M=2048")
    h.close()


def test_partial_outputs(engine_lib):
    """any subset of the four outputs: the same bits as in the full call"""
    pr = problem(O.SE_ARD, 1100, 6, 2)
    V, _ = reference(pr, 70)
    h = model(engine_lib, pr)
    full = dict(zip(NAMES, h.query_batch_grad(V)))
    for want in (("dkta",), ("dvar",), ("kta", "dvar"), ("var", "dkta"), ()):
        got = dict(zip(NAMES, h.query_batch_grad(V, want=want)))
        for k in NAMES:
            assert (got[k] is None) == (k not in want)
            if k in want:
                assert np.array_equal(got[k], full[k]), (want, k)
    h.close()


def test_grown_model(engine_lib):
    """N = 300, five add_sample calls, one add_samples(q = 70): parity on the result"""
    pr = problem(O.SE_ARD, 375, 6, 1)
    V, ref = reference(pr, 70)
    X, om = pr["X"], pr["om"]
    h = model(engine_lib, pr, 300)
    for n in range(300, 305):
        assert h.add_sample(X[n], om[:n + 1]) == 0
    assert h.add_samples(X[305:375], om) == 0
    check(h.query_batch_grad(V), ref, "grown to 375")
    h.close()


@pytest.mark.parametrize("N", [200, 1100])
def test_bitwise(engine_lib, N):
    pr = problem(O.SE_ARD, N, 6, 2)
    V700, _ = reference(pr, 700)
    h = model(engine_lib, pr)
    epoch0, ll0 = h.epoch(), h.log_lik()
    k0, v0 = h.query_batch(V700)
    a = h.query_batch_grad(V700)
    b = h.query_batch_grad(V700)
    for name, x, y in zip(NAMES, a, b):
        assert np.array_equal(x, y), f"{name}: the call repeated gives the same bits"
    sub = h.query_batch_grad(V700[300:370])
    for name, x, y in zip(NAMES, sub, a):
        assert np.array_equal(x, y[300:370]), f"{name}: seventy points alone and inside 700 give the same bits"
    k70, v70 = h.query_batch(V700[300:370])
    assert np.array_equal(sub[0], k70) and np.array_equal(sub[1], v70), "kta and var are bitwise query_batch's for M = 70"
    assert np.array_equal(a[0], k0) and np.array_equal(a[1], v0)
    assert h.epoch() == epoch0, "gpe_epoch does not move"
    assert h.log_lik() == ll0
    k1, v1 = h.query_batch(V700)
    assert np.array_equal(k1, k0) and np.array_equal(v1, v0), "a later query_batch answers bitwise what it answered before"
    h.close()


def test_statuses(engine_lib):
    GPE_ERR_ARG, GPE_ERR_STATE, GPE_ERR_UNSUPPORTED = -1, -2, -5
    fn = engine_lib.fn("query_batch_grad")
    pr = problem(O.SE_ARD, 300, 3, 1)
    X, om = pr["X"], pr["om"]
    V = np.ascontiguousarray(X[:5] + 0.01)
    out = [np.zeros(5), np.zeros(5), np.zeros(15), np.zeros(15)]
    ptr = [_capi._d(o) for o in out]
    h = _capi.Handle(engine_lib)
    h.set_data(X, om)
    h.set_kernel(O.SE_ARD, pr["th"], NOISE)
    assert fn(h._h, _capi._d(V), 5, *ptr) == GPE_ERR_STATE, "before gpe_compute"
    assert h.compute() == 0
    assert fn(h._h, _capi._d(V), -1, *ptr) == GPE_ERR_ARG
    assert fn(h._h, None, 5, *ptr) == GPE_ERR_ARG
    assert fn(h._h, None, 0, *ptr) == 0, "M = 0 returns 0 and does nothing"
    assert fn(h._h, _capi._d(V), 5, None, None, None, None) == 0, "all four outputs NULL is allowed"
    assert all(not o.any() for o in out)
    assert fn(h._h, _capi._d(V), 5, *ptr) == 0
    assert out[2].any() and out[3].any()
    ms = np.zeros(3)
    assert engine_lib.fn("query_grad_phase_ms")(h._h, _capi._d(ms)) == 0
    h.close()
    # a handle whose kernel matrix came from the host has no device code for the kernel, hence none for its derivative
    K = O.kernel_matrix(O.SE_ARD, X, pr["th"], NOISE)
    h = _capi.Handle(engine_lib)
    h.set_data(X, om)
    h.set_kernel(_capi.KERNEL_HOST_K, np.zeros(0), NOISE)
    h.set_K_host(K)
    assert h.compute() == 0
    assert fn(h._h, _capi._d(V), 5, *ptr) == GPE_ERR_UNSUPPORTED
    h.close()


# ------------------------------------------------------------------------------------------------ the C++ drop-in on the device
from tests import test_query_grad_host as H  # noqa: E402  (the driver's builder, protocol and numpy reference)


@pytest.mark.parametrize("kind,n,env", [(O.SE_ARD, 600, {}), (O.MATERN52, 400, {}), (O.SE_ARD, 120, {"LIMBO_AMD_MIN_N_FOR_GPU": "0"})],
                         ids=["se_ard_600", "matern52_400", "se_ard_120_forced_onto_the_device"])
def test_cpp_dropin_on_the_device(tmp_path, kind, n, env):
    """query_grad_batch on a device model and on a small model forced onto the device; UCB and EI gradients against numpy"""
    drv = H.build_driver("test_query_grad_dropin")
    case = H.dropin_problem(kind, n, 3, 2 if kind == O.SE_ARD else 1, 70, 50 + n)
    out = H.run_driver(drv, "grad", H.grad_case_text(*case), tmp_path, env)
    assert out["host_resident"][0] == 0
    H.check_dropin(out, H.dropin_reference(*case))


def test_cpp_batch_grad_search(tmp_path):
    """BatchGradSearch on mu (UCB with alpha = 0) of a GP fitted to -|x - 0.3|^2 in D = 4: at least the best of a 9^4 grid evaluated by
    batch(), less 1e-9.  rprop_lockstep returns the best point seen, so the search is never worse than its own starts; the grid
    makes this a check on the gradients' direction, not on luck."""
    drv = H.build_driver("test_query_grad_dropin")
    out = H.run_driver(drv, "search", H.search_case_text(n=300), tmp_path)
    assert out["host_resident"][0] == 0
    print("grid", out["grid_best"][0], "search", out["search_value"][0], out["search_point"])
    assert out["search_value"][0] >= out["grid_best"][0] - 1e-9
