"""The three-objective expected hypervolume improvement on the device (include/gpe_ehvi3.h) and through the C++ drop-in.

The checker is never the engine: tests/ehvi3_ref.py's numpy box sums (all boxes at once, numpy's pairwise sums), whose own error
against 50-digit arithmetic is E_REF_EHVI3 (tests/test_ehvi3_host.py).  Bars:
* the box sums given equal beliefs: BAR = 16 E_REF_EHVI3 relative, the value and each of the six partials, wherever the reference is
  >= 1e-280; below that 0 <= result <= 1e-279;
* the fused call's mu and var against gpe_query_batch: 1e-10.
The kernel stages a table through LDS in pieces of 512 boxes: n = 255 and 256 (511 and 513 boxes) straddle one piece, n = 31, 32, 33
(63, 65, 67 boxes) and a tied front of exactly 64 rows one 64-lane round."""
import numpy as np
import pytest

from limbo_amd import _capi
from oracle import np_oracle as O
from tests import ehvi3_cases as C
from tests import ehvi3_ref as R
from tests.test_ehvi3_host import BAR, NOISES, check_dropin, dropin_problem, rel_err, run_driver, with_steps

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 2, 31, 32, 33, 255, 256, 300, 1024, "tied64"]
VALUES_CHUNK = 16384  # beliefs on the device at once in gpe_ehvi3_values (limbo_amd/csrc/acq.hpp: kValuesChunk)
CHUNK_NM = 8192  # candidates per chunk of a fused call in the N x M layout (acq.hpp: kKgNmChunk; fewer samples than one outer panel)


@pytest.fixture(scope="module")
def any_handle(engine_lib):
    h = _capi.Handle(engine_lib)  # (not computed, no data: the box sums need the device only)
    yield h
    h.close()


def front_for(n, rng):
    if n == "tied64":
        F = C.lattice_front_with_boxes(64)
        assert len(R.boxes3(F, C.REF3, 2)) == 64
        return F
    F = C.sphere_front(n, rng)
    assert [len(R.boxes3(F, C.REF3, c)) for c in range(3)] == [2 * n + 1] * 3
    return F


def errors(v, p, rv, rp):
    return rel_err(v, rv), [rel_err(p[:, k], rp[:, k]) for k in range(6)]


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
@pytest.mark.parametrize("n", SIZES)
def test_values(any_handle, n):
    h = any_handle
    rng = np.random.default_rng(100 + (n if n != "tied64" else 64))
    F = front_for(n, rng)
    mu, s = C.near_beliefs(F, 257, rng)
    rv, rp = R.ref_ehvi3(F, C.REF3, mu, s)  # once: the smaller batches are its first candidates
    assert np.mean(rv >= 1e-280) >= 0.8 and np.mean(rv >= 1e-6) >= 0.2, "the candidates lie within 6 standard deviations of the front"
    for M in (1, 5, 257):
        rc, v, p = h.ehvi3_values(F, C.REF3, mu[:M], s[:M])
        assert rc == 0
        ev, ep = errors(v, p, rv[:M], rp[:M])
        print(f"n = {len(F)} M = {M}: ehvi in [{rv[:M].min():.3e}, {rv[:M].max():.3e}], relative error: value {ev:.3e}, partials "
              + " ".join(f"{e:.3e}" for e in ep))
        assert ev <= BAR and max(ep) <= BAR
        _, v2, p2 = h.ehvi3_values(F, C.REF3, mu[:M], s[:M])
        assert np.array_equal(v, v2) and np.array_equal(p, p2), "two calls are bitwise equal"
        _, v2, p2 = h.ehvi3_values(F, C.REF3, mu[:M], s[:M], want_partials=False)
        assert np.array_equal(v, v2) and p2 is None, "partials = NULL: the same values"
        for m in sorted({0, M // 2, M - 1}):
            _, v1, p1 = h.ehvi3_values(F, C.REF3, mu[m:m + 1], s[m:m + 1])
            assert v1[0] == v[m] and np.array_equal(p1[0], p[m]), f"candidate {m} alone"
        if M > 1:
            cut = M // 2 | 1
            lo, hi = h.ehvi3_values(F, C.REF3, mu[:cut], s[:cut]), h.ehvi3_values(F, C.REF3, mu[cut:M], s[cut:M])
            assert np.array_equal(np.concatenate([lo[1], hi[1]]), v) and np.array_equal(np.vstack([lo[2], hi[2]]), p), "two parts are the batch"
    assert np.mean(v >= 1e-6) >= 0.2, "a kernel that returns zeros must not pass"


def test_values_second_chunk(any_handle):
    h = any_handle
    rng = np.random.default_rng(33)
    F = front_for(33, rng)
    M = VALUES_CHUNK + 3
    mu, s = C.near_beliefs(F, M, rng)
    rc, v, p = h.ehvi3_values(F, C.REF3, mu, s)
    assert rc == 0 and not np.any(np.isnan(v)) and not np.any(np.isnan(p))
    _, vt, pt = h.ehvi3_values(F, C.REF3, mu[VALUES_CHUNK:], s[VALUES_CHUNK:])
    assert np.array_equal(v[VALUES_CHUNK:], vt) and np.array_equal(p[VALUES_CHUNK:], pt), "the second chunk's candidates asked alone"
    for m in (VALUES_CHUNK - 1, VALUES_CHUNK):
        _, v1, p1 = h.ehvi3_values(F, C.REF3, mu[m:m + 1], s[m:m + 1])
        assert v1[0] == v[m] and np.array_equal(p1[0], p[m]), f"candidate {m} alone"
    tail = slice(VALUES_CHUNK - 40, M)
    rv, rp = R.ref_ehvi3(F, C.REF3, mu[tail], s[tail])
    ev, ep = errors(v[tail], p[tail], rv, rp)
    assert ev <= BAR and max(ep) <= BAR


# ------------------------------------------------------------------------------------------------ 2. special inputs
@pytest.mark.parametrize("n", [0, 33])
def test_values_special_inputs(any_handle, n):
    h = any_handle
    rng = np.random.default_rng(200 + n)
    F = front_for(n, rng)
    mu0, s0 = C.near_beliefs(F, 24, rng)
    _, v0, p0 = h.ehvi3_values(F, C.REF3, mu0, s0)
    mu, s = mu0.copy(), s0.copy()
    s[0, 0] = 0.0  # s = 0 in one, two and all three objectives: the limits
    s[1, :2] = 0.0
    s[2, :] = 0.0
    mu[3, 1] = np.nan  # a NaN mean, a NaN s
    s[4, 2] = np.nan
    mu[5, 0] = np.inf
    mu[6, :] = np.inf
    mu[7, 2] = -np.inf
    mu[8, 0] = C.REF3[0] - 1e8 * s[8, 0]  # z = -1e8 and -1e100 at the reference point
    mu[9, 0] = C.REF3[0] - 1e100 * s[9, 0]
    mu[10, :] = -np.inf
    s[11, :] = 0.0
    mu[11, :] = np.inf
    mu[12], s[12] = (C.REF3[0] - 21.0 * 0.02, 0.9, 1.1), (0.02, 0.05, 0.04)  # far inside the dominated region: held relatively
    touched = np.arange(24) < 13
    rc, v, p = h.ehvi3_values(F, C.REF3, mu, s)
    assert rc == 0
    assert np.array_equal(v[~touched], v0[~touched]) and np.array_equal(p[~touched], p0[~touched]), "the other candidates are untouched"
    rv, rp = R.ref_ehvi3(F, C.REF3, mu[:3], s[:3])
    ev, ep = errors(v[:3], p[:3], rv, rp)
    print(f"n = {n}, s = 0 in one, two, three objectives: values {v[:3]}, relative error {ev:.3e}, partials {max(ep):.3e}")
    assert ev <= BAR and max(ep) <= BAR
    rv, rp = R.ref_ehvi3(F, C.REF3, mu[12:13], s[12:13])
    ev, ep = errors(v[12:13], p[12:13], rv, rp)
    print(f"n = {n}, 21 standard deviations below ref in f1: value {v[12]:.3e}, relative error {ev:.3e}, partials {max(ep):.3e}")
    assert 1e-110 <= rv[0] <= 1e-90 and ev <= BAR and max(ep) <= BAR
    assert abs(v[2] - R.hvi_points3(F, C.REF3, mu[2:3])[0]) <= 1e-15, "all three zero: the plain hypervolume improvement of the point mu"
    assert np.all(p[2, 1::2] == 0.0), "phi = 0 where s is"
    for m in (3, 4):
        assert np.isnan(v[m]) and np.all(np.isnan(p[m])), "a NaN belief gives NaN for that candidate"
    for m in (5, 6, 11):
        assert not np.isnan(v[m]) and not np.any(np.isnan(p[m])) and v[m] >= 0 and np.all(p[m] >= 0), "mu = +inf: +inf or finite, never NaN"
    assert v[6] == np.inf and v[11] == np.inf
    for m in (7, 10):
        assert v[m] == 0.0 and np.all(p[m] == 0.0), "mu = -inf gives 0"
    for m in (8, 9):
        assert v[m] == 0.0 and np.all(np.isfinite(p[m])) and np.all(p[m] >= 0), "z = -1e8, -1e100: finite"
    # a negative s: GPE_ERR_ARG, nothing written
    s[13, 1] = -1e-300
    rc, v, p = h.ehvi3_values(F, C.REF3, mu, s, check=False)
    assert rc == -1 and np.all(v == 0.0) and np.all(p == 0.0)


# ------------------------------------------------------------------------------------------------ 3. the fused call
NOISE = 0.01
KERNELS = {O.SE_ARD: np.log([0.3, 0.5, 0.8, 1.0]), O.MATERN52: np.log([0.7, 1.0])}


def fused_model(engine_lib, kind, N, P, compute=True):
    """N samples of D = 3 inputs with P noisy outputs that compete; the handle, its observations (centred) and 300 candidates"""
    rng = np.random.default_rng(1000 * kind + N + P)
    X = rng.random((N, 3))
    t = 1.5 * X.sum(axis=1)
    Y = np.stack([np.cos(t) + 0.3 * X[:, 0], np.sin(t) - 0.3 * X[:, 0], np.cos(t + 2.0) + 0.4 * X[:, 1], np.sin(2.0 * t)][:P], axis=1)
    Y = Y + 0.05 * rng.standard_normal((N, P))
    om = Y - Y.mean(axis=0)
    h = _capi.Handle(engine_lib)
    h.set_data(X, om)
    h.set_kernel(kind, KERNELS[kind], NOISE)
    if compute:
        assert h.compute() == 0
    return h, X, om, rng.uniform(-0.2, 1.2, size=(300, 3))


def front_of(om, outs, margin=0.1):
    Yo = om[:, list(outs)]
    ref = tuple(float(Yo[:, k].min()) - margin for k in range(3))
    rc, F = _capi.ehvi3_front(Yo, ref)
    assert rc == 0 and 3 <= len(F) <= _capi.EHVI3_MAX_FRONT and R.is_prepared3(F, ref)
    return F, ref


@pytest.mark.parametrize("kind,N,P,outs", [(O.SE_ARD, 200, 3, (0, 1, 2)), (O.MATERN52, 700, 4, (3, 0, 2)), (O.SE_ARD, 700, 4, (3, 0, 2)),
                                           (O.MATERN52, 200, 3, (0, 1, 2))])
def test_fused_call(engine_lib, kind, N, P, outs):
    h, X, om, V = fused_model(engine_lib, kind, N, P)
    M = len(V)
    F, ref = front_of(om, outs)
    ep0 = h.epoch()
    k0, v0 = h.query_batch(V)
    add = np.random.default_rng(5).standard_normal((M, 3)) * 0.05
    for mean_add in (None, add):
        for var_add in (0.0, NOISE):
            rc, e, p, mu, var = h.ehvi3_batch(V, F, ref, outs, mean_add, var_add)
            assert rc == 0
            want_mu = k0[:, list(outs)] + (0.0 if mean_add is None else mean_add)
            d_mu, d_var = np.max(np.abs(mu - want_mu)), np.max(np.abs(var - v0))
            sd = np.sqrt(np.where(var > np.finfo(float).eps, var, 0.0) + var_add)
            rv, rp = R.ref_ehvi3(F, ref, mu, np.stack([sd] * 3, axis=1))
            ev, epp = errors(e, p, rv, rp)
            print(f"kind {kind} N {N} outputs {outs} mean_add {mean_add is not None} var_add {var_add}: front {len(F)}, ehvi median "
                  f"{np.median(rv):.3e} max {rv.max():.3e}; max|mu - query| {d_mu:.3e}, max|var - query| {d_var:.3e}; relative error: value "
                  f"{ev:.3e}, partials {max(epp):.3e}")
            assert d_mu <= 1e-10 and d_var <= 1e-10
            assert ev <= BAR and max(epp) <= BAR
            assert np.mean(rv >= 1e-280) >= 0.8 and np.mean(e >= 1e-12) >= 0.2, "values that all vanish show little"
            cut = M // 2 | 1
            lo = h.ehvi3_batch(V[:cut], F, ref, outs, None if mean_add is None else mean_add[:cut], var_add)
            hi = h.ehvi3_batch(V[cut:], F, ref, outs, None if mean_add is None else mean_add[cut:], var_add)
            for k, full in enumerate((e, p, mu, var)):
                assert np.array_equal(np.concatenate([lo[1 + k], hi[1 + k]], axis=0), full), "two parts are bitwise the batch"
            again = h.ehvi3_batch(V, F, ref, outs, mean_add, var_add)
            assert all(np.array_equal(x, y) for x, y in zip(again[1:], (e, p, mu, var))), "two calls are bitwise equal"
            only = h.ehvi3_batch(V, F, ref, outs, mean_add, var_add, want=("ehvi",))
            assert np.array_equal(only[1], e) and only[2] is None, "partials = NULL: the same values"
    assert h.epoch() == ep0
    k1, v1 = h.query_batch(V)
    assert np.array_equal(k0, k1) and np.array_equal(v0, v1), "gpe_query_batch answers bitwise what it answered before"
    h.close()


def test_fused_second_chunk(engine_lib):
    """M = CHUNK_NM + 3 at N = 200 (the N x M layout), D = 3: the fused call runs its loop twice.  The whole batch's answers behind the
    chunk boundary are bitwise those of the same candidates asked alone, and so are the candidates on either side of the boundary."""
    h, X, om, _ = fused_model(engine_lib, O.SE_ARD, 200, 3)
    F, ref = front_of(om, (2, 0, 1))
    rng = np.random.default_rng(8192)
    M = CHUNK_NM + 3
    V, add = rng.uniform(-0.2, 1.2, size=(M, 3)), 0.05 * rng.standard_normal((M, 3))

    def call(sel):
        out = h.ehvi3_batch(V[sel], F, ref, (2, 0, 1), add[sel], NOISE)
        assert out[0] == 0
        return out[1:]

    whole = call(slice(0, M))
    assert all(w.shape[0] == M and not np.any(np.isnan(w)) for w in whole) and np.any(whole[0][CHUNK_NM:] > 0)
    for w, t in zip(whole, call(slice(CHUNK_NM, M))):
        assert np.array_equal(w[CHUNK_NM:], t), "the second chunk's candidates asked alone"
    for m in (CHUNK_NM - 1, CHUNK_NM):
        for w, o in zip(whole, call(slice(m, m + 1))):
            assert np.array_equal(w[m:m + 1], o), f"candidate {m} alone"
    h.close()


def test_status_and_phases(engine_lib, any_handle):
    h, X, om, V = fused_model(engine_lib, O.SE_ARD, 200, 3, compute=False)
    F, ref = front_of(om, (0, 1, 2))
    call = lambda front=F, r=ref, Xc=V, **kw: h.ehvi3_batch(Xc, front, r, check=False, **kw)
    written = lambda out: any(np.any(a != 0.0) for a in out[1:])
    out = call()
    assert out[0] == -2 and not written(out), "GPE_ERR_STATE before compute"
    one = (np.zeros((1, 3)), np.ones((1, 3)))
    assert h.ehvi3_values(F, ref, *one)[0] == 0, "the box sums alone need no computed model"
    assert h.compute() == 0
    ok = call()
    assert ok[0] == 0
    bad_fronts = {"unsorted": F[::-1], "a front point not above ref": np.vstack([[[ref[0], F[0, 1] + 1.0, F[0, 2] + 1.0]], F]),
                  "a duplicate": np.vstack([F[:1], F]), "n = 1025": C.sphere_front(1025, np.random.default_rng(1))}
    for what, G in bad_fronts.items():
        r = C.REF3 if what == "n = 1025" else ref
        out = call(front=G, r=r)
        assert out[0] == -1 and not written(out), what + " (batch): GPE_ERR_ARG, nothing written"
        rc, v, p = any_handle.ehvi3_values(G, r, *one, check=False)
        assert rc == -1 and v[0] == 0.0 and np.all(p == 0.0), what + " (values)"
    for kw in (dict(var_add=-1e-9), dict(var_add=float("nan")), dict(var_add=float("inf")), dict(outs=(1, 1, 2)), dict(outs=(0, 1, 3)),
               dict(outs=(-1, 1, 2)), dict(r=(np.nan, 0.0, 0.0))):
        out = call(**kw)
        assert out[0] == -1 and not written(out), kw
    assert any_handle.ehvi3_values(F, ref, np.zeros((0, 3)), np.zeros((0, 3)))[0] == 0, "M = 0"
    assert call(Xc=np.zeros((0, 3)))[0] == 0, "M = 0 is a no-op"
    h.set_profiling(True)
    assert h.ehvi3_batch(V, F, ref)[0] == 0
    ms = h.ehvi3_phase_ms()
    print(ms)
    assert set(ms) == {"solves", "kernel", "readback"} and ms["solves"] > 0 and ms["kernel"] > 0 and ms["readback"] >= 0
    h.close()
    k = _capi.Handle(engine_lib)
    k.set_data(X, om)
    k.set_kernel(_capi.KERNEL_HOST_K, np.zeros(0), NOISE)
    k.set_K_host(O.kernel_matrix(O.SE_ARD, X, KERNELS[O.SE_ARD], NOISE))
    assert k.compute() == 0
    out = k.ehvi3_batch(V, F, ref, check=False)
    assert out[0] == -5 and not written(out), "GPE_ERR_UNSUPPORTED for GPE_KERNEL_HOST_K"
    rc, v, p = k.ehvi3_values(F, ref, *one, check=False)
    assert rc == -5 and v[0] == 0.0 and np.all(p == 0.0)
    k.close()


# ------------------------------------------------------------------------------------------------ 4. the C++ drop-in on the device
@pytest.mark.parametrize("observation", [0, 1])
def test_dropin_on_the_device(tmp_path, observation):
    """N = 300 (above Params::gpu::min_n_for_gpu: through gpe_ehvi3_batch and gpe_ehvi3_values): one model with three outputs and
    three models with one output each share hyper-parameters and the Data mean, so they answer alike"""
    M = 16
    X, Y, ref, Q = dropin_problem(0, 300, M, 300 + observation)
    got = run_driver(tmp_path, 0, 0, X, Y, Y, ref, with_steps(Q), noise_id=0, observation=observation)
    assert np.all(got["host_resident"] == 0)
    got["ref_used"] = ref
    assert np.array_equal(got["front"].reshape(-1, 3), R.pareto_front3(Y, ref))
    one, three, _ = check_dropin(got, M, 3, NOISES[0], observation, BAR, f"device, observation {observation}")
    e = rel_err(got["three"], got["one"])
    print(f"the one-model form against the three-model form: {e:.3e}")
    assert e <= BAR
    assert np.mean(one >= 1e-6) >= 0.25, "values that all vanish show little"
