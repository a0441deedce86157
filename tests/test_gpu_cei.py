"""Constrained expected improvement in the log domain on the device (include/gpe_cei.h) and through the C++ drop-in.

The checker is never the engine: tests/cei_ref.py's numpy / scipy ref_logcei, whose own error against 50-digit arithmetic is E_REF_CEI
(tests/test_cei_host.py).  The measure is |got - ref| / max(1, |ref|) for values, terms and partials alike.  Bars:
* the kernel given equal beliefs: BAR = 16 E_REF_CEI, value, every term, every partial;
* the fused call's mu and var against gpe_query_batch: 1e-10;
* end to end against the CPU oracle's mu and sigma^2: 10 E_REF_CEI max(1, |ref|) + sum |partial| delta, delta = d_mu = 1e-8 for a
  mean and d_s = 1e-8 / (2 s) for a standard deviation: the project's 1e-8 parity bar on mu and sigma^2 pushed through first order,
  over candidates with |z|, |u| <= 10 (beyond, the partials grow like |z| and the bound says little).  Derived, not measured."""
import numpy as np
import pytest

from limbo_amd import _capi
from oracle import np_oracle as O
from tests import cei_ref as R
from tests.test_cei_host import BAR, E_REF_CEI, NOISES, check_dropin, dropin_problem, run_driver, with_steps
from tests.test_gpu_joint_posterior import ELL6, NOISE, problem
from tests.test_gpu_kg import CHUNK_NM, check_second_chunk, two_chunk_model
from tests.test_kg_host import dropin_reference

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def any_handle(engine_lib):
    h = _capi.Handle(engine_lib)  # (not computed, no data: the kernel alone needs the device only)
    yield h
    h.close()


def random_beliefs(M, C, rng):
    """z and u in [-30, 6]; four candidates in ten are mild (z in [-2, 6], u in [0.5, 6]) so that their logcei is above -20 whatever C"""
    mild = rng.random(M) < 0.4
    z = np.where(mild, rng.uniform(-2, 6, M), rng.uniform(-30, 6, M))
    u = np.where(mild[:, None], rng.uniform(0.5, 6, (M, C)), rng.uniform(-30, 6, (M, C)))
    s0, sc = 10 ** rng.uniform(-1.3, 0.7, M), 10 ** rng.uniform(-1.3, 0.7, (M, C))
    thr = rng.uniform(-1, 1, C)
    f_best, xi = 0.4, 0.01
    return dict(thr=thr, f_best=f_best, xi=xi, mu0=f_best + xi + z * s0, s0=s0, mu_c=thr[None, :] + u * sc, s_c=sc)


def ref_of(b, with_ei=1):
    return R.ref_logcei(with_ei, b["f_best"], b["xi"], b["thr"], b["mu0"], b["s0"], b["mu_c"], b["s_c"])


def dev_of(h, b, with_ei=1, rows=slice(None), **kw):
    rc, v, t, p = h.logcei_values(b["thr"], b["mu_c"][rows], b["s_c"][rows], b["mu0"][rows], b["s0"][rows], b["f_best"], b["xi"], with_ei, **kw)
    assert rc == 0
    return v, t, p


def errors(got, ref):
    return [float(R.err(g, r).max()) if np.size(r) else 0.0 for g, r in zip(got, ref)]


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
@pytest.mark.parametrize("C", [0, 1, 3, 16])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 257])
def test_values_random(any_handle, M, C):
    b = random_beliefs(M, C, np.random.default_rng(1000 * C + M))
    got, ref = dev_of(any_handle, b), ref_of(b)
    ev, et, ep = errors(got, ref)
    print(f"M = {M}, C = {C}: logcei in [{ref[0].min():.3e}, {ref[0].max():.3e}]; error: value {ev:.3e}, terms {et:.3e}, partials {ep:.3e}")
    assert max(ev, et, ep) <= BAR
    if M >= 63:
        assert np.mean(ref[0] > -20) >= 0.2 and np.mean(got[0] > -20) >= 0.2, "a kernel that returns -inf must not pass"
    again = dev_of(any_handle, b)
    assert all(np.array_equal(x, y) for x, y in zip(got, again)), "two calls are bitwise equal"
    v, t, p = dev_of(any_handle, b, want=())
    assert np.array_equal(v, got[0]) and t is None and p is None


def test_values_across_the_chunk(any_handle):
    """16 384 + 65 candidates: the second chunk of gpe_logcei_values"""
    M, C = 16384 + 65, 3
    b = random_beliefs(M, C, np.random.default_rng(5))
    got, ref = dev_of(any_handle, b), ref_of(b)
    ev, et, ep = errors(got, ref)
    print(f"M = {M}: error: value {ev:.3e}, terms {et:.3e}, partials {ep:.3e}")
    assert max(ev, et, ep) <= BAR and np.mean(got[0] > -20) >= 0.2
    tail = dev_of(any_handle, b, rows=slice(16384, None))
    assert all(np.array_equal(x[16384:], y) for x, y in zip(got, tail)), "the second chunk's candidates, asked alone"


# ------------------------------------------------------------------------------------------------ 2. special inputs
def test_values_special_inputs(any_handle):
    h = any_handle
    M, C = 24, 2
    b = random_beliefs(M, C, np.random.default_rng(31))
    b["mu0"] += 0.75 - b["f_best"] - b["xi"]
    b["f_best"], b["xi"] = 0.5, 0.25  # (exact in binary: mu0 - f_best - xi below is exactly the offset written)
    base = dev_of(h, b)
    # s0 = 0 on either side of the incumbent; s_k = 0 on either side of the threshold (and ON it: met)
    c = {k: np.copy(v) for k, v in b.items()}
    c["s0"][:4] = 0.0
    c["mu0"][:4] = b["f_best"] + b["xi"] + np.array([0.5, -0.5, 0.0, 2.0])
    c["s_c"][4:8, 0] = 0.0
    c["mu_c"][4:8, 0] = b["thr"][0] + np.array([0.3, -0.3, 0.0, 1e-300])
    v, t, p = dev_of(h, c)
    rv, rt, rp = ref_of(c)
    assert np.allclose(t[[0, 3], 0], np.log([0.5, 2.0]), rtol=0, atol=1e-14) and np.all(t[[1, 2], 0] == -np.inf)
    assert np.allclose(p[[0, 3], 0], [2.0, 0.5], rtol=1e-14) and np.all(p[[1, 2], 0] == 0) and np.all(p[:4, 1] == 0)
    assert np.all(t[[4, 6, 7], 1] == 0) and t[5, 1] == -np.inf and np.all(p[4:8, 2] == 0) and np.all(p[4:8, 2 + C] == 0)
    assert np.all(v[[1, 2, 5]] == -np.inf) and np.all(np.isfinite(v[[0, 3, 4, 6, 7]]))
    assert max(errors((v, t, p), (rv, rt, rp))) <= BAR
    assert all(np.array_equal(x[8:], y[8:]) for x, y in zip((v, t, p), base)), "the others are untouched"
    # with_ei = 0: the log-probability of feasibility alone; f_best and the objective's belief are not read
    v0, t0, p0 = dev_of(h, b, with_ei=0)
    assert np.all(t0[:, 0] == 0) and np.all(p0[:, :2] == 0)
    assert np.array_equal(t0[:, 1:], base[1][:, 1:]) and np.array_equal(p0[:, 2:], base[2][:, 2:])
    assert max(errors((v0, t0, p0), ref_of(b, with_ei=0))) <= BAR
    rc, v1, _, _ = h.logcei_values(b["thr"], b["mu_c"], b["s_c"], None, None, np.nan, np.nan, False)
    assert rc == 0 and np.array_equal(v1, v0)
    # a NaN in one candidate's belief, in each of the four arrays: NaN there, the neighbours bitwise unchanged
    for key in ("mu0", "s0", "mu_c", "s_c"):
        c = {k: np.copy(v) for k, v in b.items()}
        c[key][5] = np.nan
        v, t, p = dev_of(h, c)
        keep = np.arange(M) != 5
        assert np.isnan(v[5]), key
        assert all(np.array_equal(x[keep], y[keep]) for x, y in zip((v, t, p), base)), key
    # z = -1e8 (and u = -1e8): finite, and what the reference says
    c = {k: np.copy(v) for k, v in b.items()}
    c["mu0"][:3] = b["f_best"] + b["xi"] - 1e8 * b["s0"][:3]
    c["mu_c"][3:6, 1] = b["thr"][1] - 1e8 * b["s_c"][3:6, 1]
    got = dev_of(h, c)
    assert all(np.all(np.isfinite(x[:6])) for x in got) and np.all(got[0][:6] < -4e15)
    assert max(errors(got, ref_of(c))) <= BAR
    # 1e100 standard deviations away: still finite
    c["mu0"][:3] = -1e100 * b["s0"][:3]
    c["mu_c"][3:6, 1] = -1e100 * b["s_c"][3:6, 1]
    got = dev_of(h, c)
    assert all(np.all(np.isfinite(x)) for x in got)
    # +-inf means: never NaN; -inf is -inf, +inf in the objective is +inf, +inf in a constraint is a constraint surely met
    for key, col, val, want in (("mu0", None, -np.inf, -np.inf), ("mu0", None, np.inf, np.inf), ("mu_c", 0, -np.inf, -np.inf), ("mu_c", 0, np.inf, None)):
        c = {k: np.copy(v) for k, v in b.items()}
        if col is None:
            c[key][:] = val
        else:
            c[key][:, col] = val
        v, t, p = dev_of(h, c)
        assert not np.any(np.isnan(v)) and not np.any(np.isnan(t)), (key, val)
        if want is not None:
            assert np.all(v == want), (key, val)
        else:
            assert np.all(t[:, 1] == 0) and np.all(p[:, 2] == 0) and np.all(p[:, 2 + C] == 0) and np.all(np.isfinite(v))


# ------------------------------------------------------------------------------------------------ 3. batch invariance
@pytest.mark.parametrize("C", [0, 3, 16])
def test_batch_invariance(any_handle, C):
    b = random_beliefs(257, C, np.random.default_rng(40 + C))
    full = dev_of(any_handle, b)
    part = dev_of(any_handle, b, rows=slice(0, 65))
    assert all(np.array_equal(x[:65], y) for x, y in zip(full, part)), "in 65 as in 257"
    for m in (0, 7, 63, 64):
        one = dev_of(any_handle, b, rows=slice(m, m + 1))
        assert all(np.array_equal(x[m:m + 1], y) for x, y in zip(full, one)), f"candidate {m} alone"


# ------------------------------------------------------------------------------------------------ 4. the fused path
def multi_handle(engine_lib, pr, C, compute=True):
    """a handle over the problem's samples with 1 + C outputs: the problem's first, then C other directions of the same inputs"""
    rng = np.random.default_rng(77)
    cols = [pr["om"][:, 0]]
    for k in range(C):
        y = np.cos(3.0 * pr["X"] @ rng.random(pr["D"])) + 0.1 * rng.standard_normal(pr["N"])
        cols.append(y - y.mean())
    om = np.stack(cols, axis=1)
    h = _capi.Handle(engine_lib)
    h.set_data(pr["X"], om)
    h.set_kernel(pr["kind"], pr["th"], NOISE)
    if compute:
        assert h.compute() == 0
    return h, om


@pytest.mark.parametrize("name,C", [("se_ard_300x65_p2", 1), ("se_ard_300x65_p2", 3), ("matern52_1700x700", 2)])
def test_fused_path(engine_lib, oracle_lib, any_handle, name, C):
    pr = problem(name, oracle_lib)
    h, om = multi_handle(engine_lib, pr, C)
    V, M = pr["V"], pr["M"]
    ep0 = h.epoch()
    k0, v0 = h.query_batch(V)
    thr = np.linspace(-0.2, 0.2, C)
    f_best = float(np.sort(om[:, 0])[-10])
    add = np.random.default_rng(5).standard_normal((M, 1 + C)) * 0.05
    outs = list(range(1, 1 + C))
    for out0, con, mean_add, var_add, with_ei in ((0, outs, None, 0.0, 1), (0, outs, add, NOISE, 1), (C, [0] + outs[:-1], add, 0.3, 1), (0, outs, None, 0.0, 0)):
        rc, lc, t, p, mu, var = h.logcei_batch(V, thr, con, out0, f_best, 0.01, with_ei, mean_add, var_add)
        assert rc == 0
        want_mu = k0[:, [out0] + list(con)] + (0.0 if mean_add is None else mean_add)
        d_mu, d_var = np.max(np.abs(mu - want_mu)), np.max(np.abs(var - v0))
        sd = np.sqrt(np.where(var > EPS, var, 0.0) + var_add)
        sdc = np.tile(sd[:, None], (1, C))
        ref = R.ref_logcei(with_ei, f_best, 0.01, thr, mu[:, 0], sd, mu[:, 1:], sdc)
        er = max(errors((lc, t, p), ref))
        rc, lc2, t2, p2 = any_handle.logcei_values(thr, mu[:, 1:], sdc, mu[:, 0], sd, f_best, 0.01, with_ei)
        ev = max(errors((lc, t, p), (lc2, t2, p2)))
        print(f"{name} C = {C} objective {out0} var_add {var_add} with_ei {with_ei}: logcei median {np.median(lc):.3e} max {lc.max():.3e}; "
              f"max|mu - query| {d_mu:.3e}, max|var - query| {d_var:.3e}; against the reference {er:.3e}, against gpe_logcei_values {ev:.3e}")
        assert d_mu <= 1e-10 and d_var <= 1e-10
        assert er <= BAR and ev <= BAR and np.all(np.isfinite(lc))
        # one candidate set split into two calls at an odd index, and one candidate alone: bitwise the whole set's answers
        cut = M // 2 | 1
        lo = h.logcei_batch(V[:cut], thr, con, out0, f_best, 0.01, with_ei, None if mean_add is None else mean_add[:cut], var_add)
        hi = h.logcei_batch(V[cut:], thr, con, out0, f_best, 0.01, with_ei, None if mean_add is None else mean_add[cut:], var_add)
        for k, full in enumerate((lc, t, p, mu, var)):
            assert np.array_equal(np.concatenate([lo[1 + k], hi[1 + k]], axis=0), full), "two parts are bitwise the batch"
        one = h.logcei_batch(V[7:8], thr, con, out0, f_best, 0.01, with_ei, None if mean_add is None else mean_add[7:8], var_add)
        assert one[1][0] == lc[7] and np.array_equal(one[3][0], p[7]), "candidate 7 alone"
    assert h.epoch() == ep0
    k1, v1 = h.query_batch(V)
    assert np.array_equal(k0, k1) and np.array_equal(v0, v1), "gpe_query_batch answers bitwise what it answered before"
    assert h.flow_retries() == 0 and h.handover_reruns() == 0
    h.close()


# ------------------------------------------------------------------------------------------------ 5. end to end
LAM5 = 0.1
_e2e = {}


def e2e_problem(oracle_lib):
    """N = 300, D = 6, SE-ARD with ELL6, kernel noise 0.1, a noisy objective and two noisy constraints of the same inputs,
    default_rng(2), 240 candidates in the box; mu (with the Data mean: the observations' mean) and sigma^2 from the CPU oracle's
    factor and alpha"""
    if not _e2e:
        rng = np.random.default_rng(2)
        N, D, M = 300, 6, 240
        X = rng.random((N, D))
        w = rng.random((3, D))
        Y = np.stack([np.sin(3.0 * X @ w[0]), np.cos(3.0 * X @ w[1]) + 0.3, np.sin(2.0 * X @ w[2])], axis=1) + 0.1 * rng.standard_normal((N, 3))
        V = rng.random((M, D))
        Sig, mu = dropin_reference(oracle_lib, O.SE_ARD, 0, X, Y, V, LAM5, th=ELL6)
        _e2e.update(X=X, Y=Y, V=V, mu=mu, var=np.diag(Sig).copy(), M=M, D=D, thr=np.array([0.2, 0.1]), f_best=float(np.sort(Y[:, 0])[-20]))
    return _e2e


def e2e_bound(ref, part, sd, C):
    """10 E_REF_CEI max(1, |ref|) + sum |partial| delta: d_mu = 1e-8 on every mean, d_s = 1e-8 / (2 s) on every standard deviation"""
    d_mu, d_s = 1e-8, 1e-8 / (2.0 * sd)
    a = np.abs(part)
    return 10 * E_REF_CEI * np.maximum(1.0, np.abs(ref)) + d_mu * (a[:, 0] + a[:, 2:2 + C].sum(axis=1)) + d_s * (a[:, 1] + a[:, 2 + C:].sum(axis=1))


@pytest.mark.parametrize("var_add", [0.0, LAM5])
def test_end_to_end(engine_lib, oracle_lib, var_add):
    pr = e2e_problem(oracle_lib)
    C, thr, f_best = 2, pr["thr"], pr["f_best"]
    sd = np.sqrt(np.where(pr["var"] > EPS, pr["var"], 0.0) + var_add)
    sdc = np.tile(sd[:, None], (1, C))
    rv, rt, rp = R.ref_logcei(1, f_best, 0.0, thr, pr["mu"][:, 0], sd, pr["mu"][:, 1:], sdc)
    z = (pr["mu"][:, 0] - f_best) / sd
    u = (pr["mu"][:, 1:] - thr[None, :]) / sd[:, None]
    keep = (np.abs(z) <= 10) & np.all(np.abs(u) <= 10, axis=1)
    print(f"var_add {var_add}: {keep.sum()} of {pr['M']} candidates with |z|, |u| <= 10; reference logcei median {np.median(rv[keep]):.3e}, max {rv[keep].max():.3e}")
    assert keep.sum() >= 100 and np.median(rv[keep]) > -60, "a bound that means something, on values that are not all -inf"
    h = _capi.Handle(engine_lib)
    mval = pr["Y"].mean(axis=0)
    h.set_data(pr["X"], pr["Y"] - mval)
    h.set_kernel(O.SE_ARD, ELL6, LAM5)
    assert h.compute() == 0
    rc, lc, t, p, mu, var = h.logcei_batch(pr["V"], thr, [1, 2], 0, f_best, 0.0, True, np.tile(mval, (pr["M"], 1)), var_add)
    bound = e2e_bound(rv, rp, sd, C)
    d = np.abs(lc - rv)
    print(f"max|mu - oracle| {np.max(np.abs(mu - pr['mu'])):.3e}, max|var - oracle| {np.max(np.abs(var - pr['var'])):.3e}, "
          f"max|logcei - ref| {d[keep].max():.3e}, worst share of the bound {np.max(d[keep] / bound[keep]):.3e}")
    assert rc == 0 and np.all(d[keep] <= bound[keep])
    assert int(np.argmax(lc)) == int(np.argmax(rv))
    h.close()


# ------------------------------------------------------------------------------------------------ 6. statuses
def test_status_and_phases(engine_lib, oracle_lib, any_handle):
    pr = problem("se_ard_300x65_p2", oracle_lib)
    V, C = pr["V"], 2
    h, om = multi_handle(engine_lib, pr, C, compute=False)
    thr = np.zeros(C)
    call = lambda thr=thr, con=(1, 2), out0=0, Xc=V, **kw: h.logcei_batch(Xc, thr, con, out0, check=False, **kw)
    assert call()[0] == -2, "GPE_ERR_STATE before compute"
    assert h.logcei_values(thr, [[0.0, 0.0]], [[1.0, 1.0]], [0.0], [1.0])[0] == 0, "the kernel alone needs no computed model"
    assert h.compute() == 0
    ok = call()
    assert ok[0] == 0

    def refused(out, what):
        assert out[0] == -1 and all(np.all(x == 0.0) for x in out[1:]), what + ": GPE_ERR_ARG, nothing written"

    refused(call(con=(1, 1)), "a constraint output twice")
    refused(call(con=(0, 1)), "the objective's output among the constraints")
    refused(call(con=(1, 3)), "an output outside [0, P)")
    refused(call(con=(1, -1)), "a negative output")
    refused(call(out0=3), "the objective outside [0, P)")
    for bad in (np.inf, np.nan):
        refused(call(thr=np.array([0.0, bad])), "a threshold that is not finite")
        refused(call(f_best=bad), "an f_best that is not finite")
        assert call(f_best=bad, with_ei=False)[0] == 0, "f_best is not read without with_ei"
        assert call(var_add=bad)[0] == -1
    refused(call(var_add=-1e-9), "a negative var_add")
    # C = 17 needs no such model: the count is refused first
    rc = h.lib.fn("logcei_batch")(h._h, 1, 0, 0.0, 0.0, 17, np.arange(17, dtype=np.int32).ctypes.data_as(_capi.C.POINTER(_capi.C.c_int)),
                                  _capi._d(np.zeros(17)), _capi._d(np.ascontiguousarray(V)), len(V), None, 0.0, None, None, None, None, None)
    assert rc == -1, "C = 17"
    rc, v, _, _ = any_handle.logcei_values(np.zeros(17), np.zeros((1, 17)), np.ones((1, 17)), [0.0], [1.0], check=False)
    assert rc == -1 and v[0] == 0.0, "C = 17 (values)"
    rc, v, _, _ = any_handle.logcei_values(thr, [[0.0, 0.0]], [[1.0, -1.0]], [0.0], [1.0], check=False)
    assert rc == -1 and v[0] == 0.0, "a negative s"
    assert any_handle.logcei_values(thr, [[0.0, 0.0]], [[1.0, 1.0]], [0.0], [-1.0], check=False)[0] == -1, "a negative s0"
    assert any_handle.logcei_values(thr, np.zeros((0, 2)), np.zeros((0, 2)), [], [])[0] == 0, "M = 0"
    assert call(Xc=np.zeros((0, pr["D"])))[0] == 0, "M = 0 is a no-op"
    # NULL outputs: what is asked for is bitwise what the full call gives
    names = ("logcei", "terms", "partials", "mu", "var")
    for mask in (1, 2, 4, 9, 16, 30):
        want = tuple(n for k, n in enumerate(names) if mask >> k & 1)
        got = h.logcei_batch(V, thr, (1, 2), want=want)
        for k, n in enumerate(names):
            assert (got[1 + k] is None) if n not in want else np.array_equal(got[1 + k], ok[1 + k])
    h.set_profiling(True)
    assert h.logcei_batch(V, thr, (1, 2))[0] == 0
    ms = h.cei_phase_ms()
    print(ms)
    assert set(ms) == {"solves", "kernel", "readback"} and ms["solves"] > 0 and ms["kernel"] > 0 and ms["readback"] >= 0
    h.close()
    k = _capi.Handle(engine_lib)
    k.set_data(pr["X"], pr["om"])
    k.set_kernel(_capi.KERNEL_HOST_K, np.zeros(0), NOISE)
    k.set_K_host(O.kernel_matrix(pr["kind"], pr["X"], pr["th"], NOISE))
    assert k.compute() == 0
    assert k.logcei_batch(V, [0.0], [1], check=False)[0] == -5, "GPE_ERR_UNSUPPORTED for GPE_KERNEL_HOST_K"
    assert k.logcei_values([0.0], [[0.0]], [[1.0]], [0.0], [1.0], check=False)[0] == -5
    k.close()


# ------------------------------------------------------------------------------------------------ 7. the C++ drop-in on the device
def test_dropin_on_the_device(tmp_path):
    """N = 300 (above Params::gpu::min_n_for_gpu: through gpe_logcei_batch and gpe_logcei_values): one model with three outputs, and an
    objective model beside a separate constraint model; both against the host reference on the beliefs the driver reports"""
    M, D, n, C = 16, 6, 300, 2
    X, Y, thr, Q = dropin_problem(D, n, C, M, 77)
    Q = np.clip(Q, 0.0, 1.0)
    got = run_driver(tmp_path, 0, 0, X, Y, thr, with_steps(Q), noise_id=1, observation=1, hp=ELL6)
    assert np.all(got["host_resident"] == 0) and int(got["used"][0]) == 1
    v, two = check_dropin(got, M, D, C, thr, NOISES[1], 1, BAR, "device, one model and two")
    assert np.all(np.isfinite(v)) and np.all(np.isfinite(two))


def test_search_leaves_the_plateau(tmp_path):
    """one opt::BatchGradSearch run on LogCEI over a problem whose plain ECI is exactly 0 at every start: it ends at a point whose
    logcei is above every start's (no fixed target: the search is 40 Rprop steps from 8 of 64 candidates)"""
    D, n, C = 6, 300, 2
    rng = np.random.default_rng(8)
    X, Y, thr, Q = dropin_problem(D, n, C, 4, 78)
    Y[:, 0] = -400.0 * np.sum((X - 1.0) ** 2, axis=1) + 0.05 * rng.standard_normal(n)  # a peak in the corner: the box lies far below it
    got = run_driver(tmp_path, 0, 0, X, Y, thr, np.clip(Q, 0.0, 1.0), noise_id=1, observation=1, hp=ELL6, search=1)
    assert np.all(got["host_resident"] == 0)
    lc, eci = got["search_starts_logcei"], got["search_starts_eci"]
    starts = np.argsort(-lc, kind="stable")[:8]
    print(f"logcei at the 8 starts {np.sort(lc[starts])}, plain ECI there {eci[starts]}; after the search {got['search_value'][0]:.6e}")
    assert len(lc) == 64 and np.all(np.isfinite(lc)) and np.all(eci[starts] == 0.0), "plain ECI is exactly 0 at every start"
    assert got["search_value"][0] > lc.max(), "the search climbs where the plain value is flat"


# ------------------------------------------------------------------------------------------------ the fused call's second chunk
def test_fused_second_chunk(engine_lib):
    h, V, rng = two_chunk_model(engine_lib, 3)
    add = 0.05 * rng.standard_normal((len(V), 3))

    def call(sel):
        out = h.logcei_batch(V[sel], [-0.2, 0.1], [1, 2], out0=0, f_best=0.5, with_ei=True, mean_add=add[sel], var_add=0.1)
        assert out[0] == 0
        return out[1:]

    check_second_chunk(call, len(V))
    assert np.all(np.isfinite(call(slice(CHUNK_NM, len(V)))[0]))
    h.close()
