"""Max-value entropy search in the log domain on the device (include/gpe_mes.h) and through the C++ drop-in.

The checker is never the engine: tests/mes_ref.py's numpy / scipy ref_mes, whose own error against 60-digit arithmetic is E_REF_MES
(tests/test_mes_host.py).  The measure is |got - ref| / max(1, |ref|) for values, terms and partials alike.  Bars:
* the kernel given equal beliefs: BAR = 16 E_REF_MES, value, every term, every partial;
* the fused call's mu and var against gpe_query_batch: 1e-10;
* end to end against the CPU oracle's mu and sigma^2: 10 E_REF_MES max(1, |ref|) + sum |partial| delta, delta = d_mu = 1e-8 for a
  mean and d_s = 1e-8 / (2 s) for a standard deviation: the project's 1e-8 parity bar on mu and sigma^2 pushed through first order,
  over candidates with |g| <= 10 (test_gpu_cei.py's bound).  Derived, not measured."""
import numpy as np
import pytest

from limbo_amd import _capi
from oracle import np_oracle as O
from tests import mes_ref as R
from tests.test_gpu_cei import multi_handle
from tests.test_gpu_joint_posterior import ELL6, NOISE, problem
from tests.test_gpu_kg import CHUNK_NM, check_second_chunk, two_chunk_model
from tests.test_kg_host import dropin_reference
from tests.test_mes_host import BAR, E_REF_MES, NOISES, check_dropin, dropin_problem, run_driver, with_steps

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def any_handle(engine_lib):
    h = _capi.Handle(engine_lib)  # (not computed, no data: the kernel alone needs the device only)
    yield h
    h.close()


def beliefs(M, K, J, rng):
    """per candidate a centre c ~ U[-30, 12] and g_jk = c + d_kj, d ~ U[-1.5, 1.5]: the samples are shared by the candidates, so
    output j has one s_j for all of them (10^U[-1.3, 0.7]) and ystar_kj = y0_j + d_kj s_j, mu_mj = y0_j - c_m s_j"""
    c = rng.uniform(-30, 12, M)
    s_ref = 10 ** rng.uniform(-1.3, 0.7, J)
    d = rng.uniform(-1.5, 1.5, (K, J))
    ystar = rng.uniform(-1, 1, J)[None, :] + d * s_ref[None, :]
    s = np.tile(s_ref[None, :], (M, 1))
    mu = (ystar[0] - d[0] * s_ref)[None, :] - c[:, None] * s
    return dict(ystar=ystar, mu=mu, s=s)


def ref_of(b, rows=slice(None)):
    return R.ref_mes(b["ystar"], b["mu"][rows], b["s"][rows])


def dev_of(h, b, rows=slice(None), **kw):
    rc, v, t, p = h.mes_values(b["ystar"], b["mu"][rows], b["s"][rows], **kw)
    assert rc == 0
    return v, t, p


def errors(got, ref):
    return [float(R.err(g, r).max()) if np.size(r) else 0.0 for g, r in zip(got, ref)]


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
@pytest.mark.parametrize("J", [1, 2, 8])
@pytest.mark.parametrize("K", [1, 10, 63, 64, 65, 1024])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 257])
def test_values_random(any_handle, M, K, J):
    b = beliefs(M, K, J, np.random.default_rng(100000 * J + 100 * K + M))
    got, ref = dev_of(any_handle, b), ref_of(b)
    ev, et, ep = errors(got, ref)
    print(f"M = {M}, K = {K}, J = {J}: logmes in [{ref[0].min():.3e}, {ref[0].max():.3e}]; error: value {ev:.3e}, terms {et:.3e}, partials {ep:.3e}")
    assert max(ev, et, ep) <= BAR
    if M >= 63:
        assert np.mean(ref[0] > -20) >= 0.2 and np.mean(got[0] > -20) >= 0.2, "a kernel that returns -inf must not pass"
    again = dev_of(any_handle, b)
    assert all(np.array_equal(x, y) for x, y in zip(got, again)), "two calls are bitwise equal"
    v, t, p = dev_of(any_handle, b, want=())
    assert np.array_equal(v, got[0]) and t is None and p is None
    _, t1, p1 = dev_of(any_handle, b, want=("terms",))
    _, t2, p2 = dev_of(any_handle, b, want=("partials",))
    assert np.array_equal(t1, got[1]) and p1 is None and t2 is None and np.array_equal(p2, got[2]), "outputs asked for or not"


def test_values_across_the_chunk(any_handle):
    """16 384 + 65 candidates: the second chunk of gpe_mes_values"""
    M, K, J = 16384 + 65, 10, 2
    b = beliefs(M, K, J, np.random.default_rng(5))
    got, ref = dev_of(any_handle, b), ref_of(b)
    ev, et, ep = errors(got, ref)
    print(f"M = {M}: error: value {ev:.3e}, terms {et:.3e}, partials {ep:.3e}")
    assert max(ev, et, ep) <= BAR and np.mean(got[0] > -20) >= 0.2
    tail = dev_of(any_handle, b, rows=slice(16384, None))
    assert all(np.array_equal(x[16384:], y) for x, y in zip(got, tail)), "the second chunk's candidates, asked alone"


# ------------------------------------------------------------------------------------------------ 2. special inputs
def test_values_special_inputs(any_handle):
    h = any_handle
    M, K, J = 24, 5, 3
    b = beliefs(M, K, J, np.random.default_rng(31))
    base = dev_of(h, b)
    copy = lambda: {k: np.copy(v) for k, v in b.items()}
    # s_j = 0: the term is -inf and its partials are 0, whatever the order of mu and ystar; the other outputs go on
    c = copy()
    c["s"][:3, 1] = 0.0
    c["mu"][:3, 1] = [b["ystar"][:, 1].min() - 1.0, b["ystar"][:, 1].max() + 1.0, b["ystar"][0, 1]]
    v, t, p = dev_of(h, c)
    assert np.all(t[:3, 1] == -np.inf) and np.all(p[:3, 1] == 0) and np.all(p[:3, J + 1] == 0) and np.all(np.isfinite(v[:3]))
    assert max(errors((v, t, p), ref_of(c))) <= BAR
    assert all(np.array_equal(x[3:], y[3:]) for x, y in zip((v, t, p), base)), "the others are untouched"
    # every s = 0: logmes = -inf, the partials 0
    c = copy()
    c["s"][:2] = 0.0
    v, t, p = dev_of(h, c)
    assert np.all(v[:2] == -np.inf) and np.all(t[:2] == -np.inf) and np.all(p[:2] == 0)
    # a NaN in one candidate's belief: NaN there (value, terms, partials), the neighbours bitwise unchanged
    for key in ("mu", "s"):
        c = copy()
        c[key][5, 2] = np.nan
        v, t, p = dev_of(h, c)
        keep = np.arange(M) != 5
        assert np.isnan(v[5]) and np.all(np.isnan(t[5])) and np.all(np.isnan(p[5])), key
        assert all(np.array_equal(x[keep], y[keep]) for x, y in zip((v, t, p), base)), key
    # |g| = 1e8: finite, and what the reference says; 1e100: finite, and the asymptotes
    c = copy()
    c["mu"][:3, 0] = b["ystar"][0, 0] + 1e8 * b["s"][:3, 0]
    c["mu"][3:6, 1] = b["ystar"][0, 1] - 1e8 * b["s"][3:6, 1]
    got = dev_of(h, c)
    assert all(np.all(np.isfinite(x[:6])) for x in got)
    assert max(errors(got, ref_of(c))) <= BAR
    x = 1e100
    for sg in (-1.0, 1.0):
        y1 = np.array([[0.0]])
        rc, v, t, p = h.mes_values(y1, [[-sg * x * 0.5]], [[0.5]])
        rv, rt, rp = R.ref_mes(y1, [[-sg * x * 0.5]], [[0.5]])
        assert rc == 0 and np.isfinite(v[0]) and np.all(np.isfinite(p)) and np.all(p != 0)
        assert max(errors((v, t, p), (rv, rt, rp))) <= BAR
    tv = np.log(x) + R.LOG_SQRT2PI - 0.5
    rc, v, t, p = h.mes_values([[0.0]], [[x]], [[1.0]])
    assert abs(v[0] - np.log(tv)) <= 1e-15 * np.log(tv) and abs(p[0, 0] - 1.0 / x / tv) <= 1e-14 / x / tv
    rc, v, t, p = h.mes_values([[0.0]], [[-x]], [[1.0]])
    assert abs(v[0] + 0.5 * x * x) <= 1e-15 * x * x and abs(p[0, 0] - x) <= 1e-14 * x
    # +-inf means: never NaN; mu = -inf: the term is -inf, mu = +inf: +inf; the partials are 0
    for val, col in ((-np.inf, None), (np.inf, None), (-np.inf, 1), (np.inf, 1)):
        c = copy()
        if col is None:
            c["mu"][:] = val
        else:
            c["mu"][:, col] = val
        v, t, p = dev_of(h, c)
        assert not np.any(np.isnan(v)) and not np.any(np.isnan(t)) and not np.any(np.isnan(p)), (val, col)
        cols = slice(None) if col is None else col
        assert np.all(t[:, cols] == val)
        if val > 0 or col is None:
            assert np.all(v == val) and np.all(p == 0)
        else:
            assert np.all(np.isfinite(v)) and np.all(p[:, col] == 0) and np.all(p[:, J + col] == 0)
        assert max(errors((v, t, p), ref_of(c))) <= BAR
    # statuses: outputs untouched
    rc, v, _, _ = h.mes_values(b["ystar"], b["mu"], -b["s"], check=False)
    assert rc == -1 and np.all(v == 0.0), "a negative s"
    bad = b["ystar"].copy()
    bad[1, 1] = np.inf
    rc, v, _, _ = h.mes_values(bad, b["mu"], b["s"], check=False)
    assert rc == -1 and np.all(v == 0.0), "a ystar that is not finite"
    assert h.mes_values(np.zeros((3, 9)), np.zeros((1, 9)), np.ones((1, 9)), check=False)[0] == -1, "J = 9"
    assert h.mes_values(np.zeros((1025, 1)), np.zeros((1, 1)), np.ones((1, 1)), check=False)[0] == -1, "K = 1025"
    assert h.mes_values(b["ystar"], np.zeros((0, J)), np.zeros((0, J)))[0] == 0, "M = 0"


# ------------------------------------------------------------------------------------------------ 3. batch invariance
@pytest.mark.parametrize("K", [1, 1024])
@pytest.mark.parametrize("J", [1, 8])
def test_batch_invariance(any_handle, J, K):
    """candidates 16 384 .. lie in the second chunk of gpe_mes_values"""
    M = 16384 + 65
    b = beliefs(M, K, J, np.random.default_rng(40 + J + K))
    full = dev_of(any_handle, b)
    part = dev_of(any_handle, b, rows=slice(0, 65))
    assert all(np.array_equal(x[:65], y) for x, y in zip(full, part)), "in 65 as in 16 449"
    for m in (0, 7, 63, 64, 16384, 16384 + 64):
        one = dev_of(any_handle, b, rows=slice(m, m + 1))
        assert all(np.array_equal(x[m:m + 1], y) for x, y in zip(full, one)), f"candidate {m} alone"


# ------------------------------------------------------------------------------------------------ 4. the fused path
def samples_for(mu, sd, K, rng, spread=1.5):
    """K sampled maxima per output a little above the best mean, by up to `spread` median standard deviations"""
    J = mu.shape[1]
    return mu.max(axis=0)[None, :] + np.median(sd) * rng.uniform(0.0, spread, (K, J))


@pytest.mark.parametrize("name,J,K", [("se_ard_300x65_p2", 1, 10), ("se_ard_300x65_p2", 3, 64), ("matern52_1700x700", 2, 65)])
def test_fused_path(engine_lib, oracle_lib, any_handle, name, J, K):
    pr = problem(name, oracle_lib)
    h, om = multi_handle(engine_lib, pr, J - 1)
    V, M = pr["V"], pr["M"]
    ep0 = h.epoch()
    k0, v0 = h.query_batch(V)
    rng = np.random.default_rng(5)
    add = rng.standard_normal((M, J)) * 0.05
    ystar = samples_for(k0, np.sqrt(np.maximum(v0, 0.0) + NOISE), K, rng)
    fwd, rev = list(range(J)), list(range(J))[::-1]
    for outs, mean_add, var_add in ((fwd, None, 0.0), (fwd, add, NOISE), (rev, add, 0.3)):
        rc, lm, t, p, mu, var = h.mes_batch(V, ystar, outs, mean_add, var_add)
        assert rc == 0
        want_mu = k0[:, outs] + (0.0 if mean_add is None else mean_add)
        d_mu, d_var = np.max(np.abs(mu - want_mu)), np.max(np.abs(var - v0))
        sd = np.tile(np.sqrt(np.where(var > EPS, var, 0.0) + var_add)[:, None], (1, J))
        ref = R.ref_mes(ystar, mu, sd)
        er = max(errors((lm, t, p), ref))
        rc, lm2, t2, p2 = any_handle.mes_values(ystar, mu, sd)
        ev = max(errors((lm, t, p), (lm2, t2, p2)))
        print(f"{name} J = {J} K = {K} outs {outs} var_add {var_add}: logmes median {np.median(lm):.3e} max {lm.max():.3e}; "
              f"max|mu - query| {d_mu:.3e}, max|var - query| {d_var:.3e}; against the reference {er:.3e}, against gpe_mes_values {ev:.3e}")
        assert d_mu <= 1e-10 and d_var <= 1e-10
        assert er <= BAR and ev <= BAR and not np.any(np.isnan(lm))
        # one candidate set split into two calls at an odd index, and one candidate alone: bitwise the whole set's answers
        cut = M // 2 | 1
        lo = h.mes_batch(V[:cut], ystar, outs, None if mean_add is None else mean_add[:cut], var_add)
        hi = h.mes_batch(V[cut:], ystar, outs, None if mean_add is None else mean_add[cut:], var_add)
        for k, full in enumerate((lm, t, p, mu, var)):
            assert np.array_equal(np.concatenate([lo[1 + k], hi[1 + k]], axis=0), full, equal_nan=True), "two parts are bitwise the batch"
        one = h.mes_batch(V[7:8], ystar, outs, None if mean_add is None else mean_add[7:8], var_add)
        assert one[1][0] == lm[7] and np.array_equal(one[3][0], p[7]), "candidate 7 alone"
    assert h.epoch() == ep0
    k1, v1 = h.query_batch(V)
    assert np.array_equal(k0, k1) and np.array_equal(v0, v1), "gpe_query_batch answers bitwise what it answered before"
    assert h.flow_retries() == 0 and h.handover_reruns() == 0
    h.close()


# ------------------------------------------------------------------------------------------------ 5. end to end
LAM5 = 0.1
_e2e = {}


def e2e_problem(oracle_lib):
    """N = 300, D = 6, SE-ARD with ELL6, kernel noise 0.1, three noisy objectives of the same inputs, default_rng(2), 240 candidates
    in the box; mu (with the Data mean: the observations' mean) and sigma^2 from the CPU oracle's factor and alpha"""
    if not _e2e:
        rng = np.random.default_rng(2)
        N, D, M = 300, 6, 240
        X = rng.random((N, D))
        w = rng.random((3, D))
        Y = np.stack([np.sin(3.0 * X @ w[0]), np.cos(3.0 * X @ w[1]) + 0.3, np.sin(2.0 * X @ w[2])], axis=1) + 0.1 * rng.standard_normal((N, 3))
        V = rng.random((M, D))
        Sig, mu = dropin_reference(oracle_lib, O.SE_ARD, 0, X, Y, V, LAM5, th=ELL6)
        _e2e.update(X=X, Y=Y, V=V, mu=mu, var=np.diag(Sig).copy(), M=M, D=D)
    return _e2e


def e2e_bound(ref, part, sd, J):
    """10 E_REF_MES max(1, |ref|) + sum |partial| delta: d_mu = 1e-8 on every mean, d_s = 1e-8 / (2 s) on every standard deviation"""
    a = np.abs(part)
    return 10 * E_REF_MES * np.maximum(1.0, np.abs(ref)) + 1e-8 * a[:, :J].sum(axis=1) + 1e-8 / (2.0 * sd) * a[:, J:].sum(axis=1)


@pytest.mark.parametrize("var_add", [0.0, LAM5])
def test_end_to_end(engine_lib, oracle_lib, var_add):
    pr = e2e_problem(oracle_lib)
    J, K = 3, 16
    sd = np.sqrt(np.where(pr["var"] > EPS, pr["var"], 0.0) + var_add)
    ystar = samples_for(pr["mu"], sd, K, np.random.default_rng(9), 0.5)  # (119 of the 240 candidates keep |g| <= 10 without the noise)
    rv, rt, rp = R.ref_mes(ystar, pr["mu"], np.tile(sd[:, None], (1, J)))
    g = (ystar.T[None, :, :] - pr["mu"][:, :, None]) / sd[:, None, None]
    keep = np.all(np.abs(g) <= 10, axis=(1, 2))
    print(f"var_add {var_add}: {keep.sum()} of {pr['M']} candidates with |g| <= 10; reference logmes median {np.median(rv[keep]):.3e}, max {rv[keep].max():.3e}")
    assert keep.sum() >= 100 and np.median(rv[keep]) > -60, "a bound that means something, on values that are not all -inf"
    h = _capi.Handle(engine_lib)
    mval = pr["Y"].mean(axis=0)
    h.set_data(pr["X"], pr["Y"] - mval)
    h.set_kernel(O.SE_ARD, ELL6, LAM5)
    assert h.compute() == 0
    rc, lm, t, p, mu, var = h.mes_batch(pr["V"], ystar, None, np.tile(mval, (pr["M"], 1)), var_add)
    bound = e2e_bound(rv, rp, sd, J)
    d = np.abs(lm - rv)
    print(f"max|mu - oracle| {np.max(np.abs(mu - pr['mu'])):.3e}, max|var - oracle| {np.max(np.abs(var - pr['var'])):.3e}, "
          f"max|logmes - ref| {d[keep].max():.3e}, worst share of the bound {np.max(d[keep] / bound[keep]):.3e}")
    assert rc == 0 and np.all(d[keep] <= bound[keep])
    assert int(np.argmax(lm)) == int(np.argmax(rv))
    h.close()


# ------------------------------------------------------------------------------------------------ 6. statuses
def test_status_and_phases(engine_lib, oracle_lib, any_handle):
    pr = problem("se_ard_300x65_p2", oracle_lib)
    V, J, K = pr["V"], 3, 7
    h, om = multi_handle(engine_lib, pr, J - 1, compute=False)
    ystar = np.random.default_rng(1).uniform(0.5, 1.5, (K, J))
    call = lambda ystar=ystar, outs=(0, 1, 2), Xc=V, **kw: h.mes_batch(Xc, ystar, outs, check=False, **kw)
    assert call()[0] == -2, "GPE_ERR_STATE before compute"
    assert h.mes_values(ystar, np.zeros((1, J)), np.ones((1, J)))[0] == 0, "the kernel alone needs no computed model"
    assert h.compute() == 0
    ep0 = h.epoch()
    k0, v0 = h.query_batch(V)
    ok = call()
    assert ok[0] == 0

    def refused(out, what):
        assert out[0] == -1 and all(np.all(x == 0.0) for x in out[1:]), what + ": GPE_ERR_ARG, nothing written"

    refused(call(outs=(0, 1, 1)), "an output twice")
    refused(call(outs=(0, 1, 3)), "an output outside [0, P)")
    refused(call(outs=(0, 1, -1)), "a negative output")
    for bad in (np.inf, -np.inf, np.nan):
        y = ystar.copy()
        y[2, 1] = bad
        refused(call(ystar=y), "a ystar that is not finite")
        assert call(var_add=bad)[0] == -1
    refused(call(var_add=-1e-9), "a negative var_add")
    refused(h.mes_batch(V, np.ones((3, 9)), list(range(9)), check=False), "J = 9")
    refused(h.mes_batch(V, np.ones((1025, 1)), [0], check=False), "K = 1025")
    assert call(Xc=np.zeros((0, pr["D"])))[0] == 0, "M = 0 is a no-op"
    # NULL outputs: what is asked for is bitwise what the full call gives
    names = ("logmes", "terms", "partials", "mu", "var")
    for mask in (1, 2, 4, 9, 16, 30):
        want = tuple(n for k, n in enumerate(names) if mask >> k & 1)
        got = h.mes_batch(V, ystar, (0, 1, 2), want=want)
        for k, n in enumerate(names):
            assert (got[1 + k] is None) if n not in want else np.array_equal(got[1 + k], ok[1 + k])
    h.set_profiling(True)
    assert h.mes_batch(V, ystar, (0, 1, 2))[0] == 0
    ms = h.mes_phase_ms()
    print(ms)
    assert set(ms) == {"solves", "kernel", "readback"} and ms["solves"] > 0 and ms["kernel"] > 0 and ms["readback"] >= 0
    h.set_profiling(False)
    assert h.epoch() == ep0
    k1, v1 = h.query_batch(V)
    assert np.array_equal(k0, k1) and np.array_equal(v0, v1), "a following gpe_query_batch is bitwise unchanged"
    h.close()
    k = _capi.Handle(engine_lib)
    k.set_data(pr["X"], pr["om"])
    k.set_kernel(_capi.KERNEL_HOST_K, np.zeros(0), NOISE)
    k.set_K_host(O.kernel_matrix(pr["kind"], pr["X"], pr["th"], NOISE))
    assert k.compute() == 0
    assert k.mes_batch(V, [[1.0]], [0], check=False)[0] == -5, "GPE_ERR_UNSUPPORTED for GPE_KERNEL_HOST_K"
    assert k.mes_values([[1.0]], [[0.0]], [[1.0]], check=False)[0] == -5
    k.close()


# ------------------------------------------------------------------------------------------------ 7. the C++ drop-in on the device
def test_dropin_on_the_device(tmp_path):
    """N = 300 (above Params::gpu::min_n_for_gpu: through gpe_mes_batch, gpe_mes_values and gpe_paths_argmax): one model with two
    outputs, against the host reference on the beliefs the driver reports"""
    M, D, n, P, K = 16, 6, 300, 2, 8
    X, Y, Q = dropin_problem(D, n, P, M, 77)
    Q = np.clip(Q, 0.0, 1.0)
    got = run_driver(tmp_path, 0, 0, X, Y, with_steps(Q), K, 11, noise_id=1, observation=1, hp=ELL6)
    assert np.all(got["host_resident"] == 0)
    check_dropin(got, M, D, P, K, NOISES[1], 1, "device")


def search_problem(D=6, n=300, seed=78):
    """a peak of height 400 in the corner of the box under a small noise: the sampled maxima lie hundreds of standard deviations
    above the mean over most of the box"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, size=(n, D))
    Y = (-400.0 * np.sum((X - 1.0) ** 2, axis=1) + 0.05 * rng.standard_normal(n))[:, None]
    return X, Y


def check_search(got, K, noise):
    """from starts where the textbook MES is exactly 0 — g > 39 for every sample, t as written 0, the plain value and its gradient
    0 — one opt::BatchGradSearch run on acqui::MES ends at a point whose logmes is above every start's (no fixed target: the search
    is 40 Rprop steps from 8 of 64 candidates)"""
    ystar = got["ystar"]
    lm, plain, pg = got["search_starts_logmes"], got["search_starts_plain"], got["search_starts_plain_grad"]
    sd = np.sqrt(got["search_s2"])  # (observation = 1)
    g = (ystar[None, :] - got["search_mu"][:, None]) / sd[:, None]
    starts = np.argsort(-lm, kind="stable")[:8]
    print(f"g at the 8 starts in [{g[starts].min():.1f}, {g[starts].max():.1f}]; logmes there {np.sort(lm[starts])}; after the search {got['search_value'][0]:.6e}")
    assert len(lm) == 64 and np.all(np.isfinite(lm))
    assert np.all(g[starts] > 39), "every sample lies more than 39 standard deviations above every start"
    with np.errstate(all="ignore"):
        assert np.all(R.textbook_t(g[starts]) == 0.0), "the textbook term is exactly 0 there"
    assert np.all(plain[starts] == 0.0) and np.all(pg.reshape(64, -1)[starts] == 0.0), "and so are the plain value and its gradient"
    assert got["search_value"][0] > lm.max(), "the search climbs where the plain value is flat"


def test_search_leaves_the_flat_region(tmp_path):
    X, Y = search_problem()
    got = run_driver(tmp_path, 0, 0, X, Y, X[:2], 8, 5, noise_id=1, observation=1, hp=ELL6, search=1)
    assert np.all(got["host_resident"] == 0)
    check_search(got, 8, NOISES[1])


# ------------------------------------------------------------------------------------------------ the fused call's second chunk
def test_fused_second_chunk(engine_lib):
    h, V, rng = two_chunk_model(engine_lib, 2)
    ystar = 1.0 + 0.3 * np.abs(rng.standard_normal((65, 2)))
    add = 0.05 * rng.standard_normal((len(V), 2))

    def call(sel):
        out = h.mes_batch(V[sel], ystar, mean_add=add[sel], var_add=0.1)
        assert out[0] == 0
        return out[1:]

    check_second_chunk(call, len(V))
    assert np.all(np.isfinite(call(slice(CHUNK_NM, len(V)))[0]))
    h.close()
