"""The knowledge gradient over a finite alternative set on the device (include/gpe_kg.h) and through the C++ drop-in.

The checker is never the engine: Sigma and mu come from the CPU oracle's factor and alpha (the cached references of
tests/test_gpu_joint_posterior.py), the envelope is tests/kg_ref.py's sorted stack algorithm — not the engine's successor chain.
Bars:
* the envelope given equal inputs: 16 E_REF relative (E_REF: the reference's own measured error against 50 digits,
  tests/test_kg_host.py; the factor covers the device's own erfc / exp and another summation order over at most A - 1 positive
  terms) wherever the reference is >= 1e-280; below that 0 <= kg <= 1e-279;
* cov and var_c against the oracle 1e-8 absolute (sigma_f = 1: the bar check_cov_and_kta holds Sigma to), var_c against
  gpe_query_batch 1e-10;
* end to end, on a problem where the knowledge gradient is large: |kg - ref| <= 2 d + 0.8 d (lambda^-1/2 + 1 / (3 sqrt(3) lambda)),
  d = 1e-8: h is 1-Lipschitz in a (twice: the envelope and the max), E|Z| <= 0.8-Lipschitz in b, and the bracket bounds how an error
  d in c and s moves b = c / sqrt(s + lambda) given |c| <= sqrt(s) at sigma_f = 1.  Derived, not measured.
On the data-rich problems of the joint posterior's tests the median knowledge gradient is below 1e-40: an absolute bar alone would
pass a kernel that returns zeros, so the inputs (cov, var_c) and the envelope given those inputs are held separately there."""
import math

import numpy as np
import pytest

from limbo_amd import _capi
from oracle import np_oracle as O
from tests import kg_cases as K
from tests import kg_ref as R
from tests.test_gpu_batch_select import small_problem
from tests.test_gpu_joint_posterior import ELL6, NOISE, model, problem
from tests.test_kg_host import E_REF, dropin_reference, rel_err, run_driver

pytestmark = pytest.mark.gpu
BAR = 16 * E_REF
SIZES = [1, 2, 3, 63, 64, 65, 257, 2048]
# name: alternatives (the first points of V; the rest are the candidates)
PROBLEMS = {"se_ard_300x65_p2": 33, "matern52_1700x700": 257, "se_ard_d20_1700x700": 257, "matern52_40x129": 33}


@pytest.fixture(scope="module")
def any_handle(engine_lib):
    h = _capi.Handle(engine_lib)  # (not computed, no data: the envelope needs the device only)
    yield h
    h.close()


def envelope(h, a, B, pad=3):
    B = np.asarray(B, dtype=np.float64).reshape(len(a), -1)
    rc, kg, nseg = h.kg_envelope(a, B, ldb=len(a) + pad)
    assert rc == 0
    return kg, nseg


def check_columns(h, a, B, what):
    B = np.asarray(B, dtype=np.float64).reshape(len(a), -1)
    kg, nseg = envelope(h, a, B)
    ref = np.array([R.ref_h(a, B[:, m]) for m in range(B.shape[1])])
    assert np.all(np.isfinite(kg)), what
    e = rel_err(kg, ref)
    print(f"A = {len(a)} {what}: h in [{ref.min():.3e}, {ref.max():.3e}], max relative error {e:.3e}")
    assert e <= BAR, what
    assert np.all(nseg >= 0) and np.all(nseg <= max(len(a) - 1, 0))
    return kg, nseg, ref


# ------------------------------------------------------------------------------------------------ 1. the envelope alone
@pytest.mark.parametrize("A", SIZES)
def test_envelope_random(any_handle, A):
    rng = np.random.default_rng(A)
    a, B = rng.standard_normal(A), rng.standard_normal((A, 65))
    kg65, nseg65, _ = check_columns(any_handle, a, B, "random, M = 65")
    kg1, nseg1, _ = check_columns(any_handle, a, B[:, 7], "random, M = 1")
    assert kg1[0] == kg65[7] and nseg1[0] == nseg65[7], "a column's answer does not depend on the batch around it"
    again, _ = envelope(any_handle, a, B)
    assert np.array_equal(again, kg65), "two calls are bitwise equal"
    if A == 1:
        assert np.all(kg65 == 0.0) and np.all(nseg65 == 0)


@pytest.mark.parametrize("A", SIZES)
def test_envelope_special_inputs(any_handle, A):
    h = any_handle
    rng = np.random.default_rng(1000 + A)
    # tangents of a parabola: every line is on the envelope
    a, b = K.parabola(A)
    _, nseg, _ = check_columns(h, a, b, "parabola")
    assert nseg[0] == A - 1
    # all slopes equal, all slopes zero: nothing to gain, exactly
    a = rng.standard_normal(A)
    kg, nseg = envelope(h, a, np.stack([np.full(A, 0.75), np.zeros(A), np.full(A, -0.0)], axis=1))
    assert np.all(kg == 0.0) and np.all(nseg == 0)
    if A >= 3:
        # a dominated middle line: below the crossing of its neighbours
        a, b = rng.standard_normal(A), np.sort(rng.standard_normal(A))
        mid = A // 2
        zx = (a[mid - 1] - a[mid + 1]) / (b[mid + 1] - b[mid - 1])  # where its neighbours in slope cross
        a[mid] = a[mid - 1] + (b[mid - 1] - b[mid]) * zx - 5.0
        kg, _, _ = check_columns(h, a, b, "dominated middle line")
        keep = np.arange(A) != mid
        assert kg[0] == envelope(h, a[keep], b[keep])[0][0], "the dominated line changes nothing, bitwise"
    if A >= 2:
        # duplicates in slope; duplicates in both a and b
        a, b = K.random_lines(A, 2000 + A)
        b[1::2] = b[0::2][: len(b[1::2])]
        check_columns(h, a, b, "duplicate slopes")
        a[1::2] = a[0::2][: len(a[1::2])]
        check_columns(h, a, b, "duplicate lines")
        # half the lines through one point; half the slopes equal; a coarse grid (exact ties)
        check_columns(h, *K.concurrent(A, 3000 + A), "concurrent lines")
        check_columns(h, *K.equal_slopes(A, 4000 + A), "half the slopes equal")
        check_columns(h, *K.grid(A, 5000 + A), "grid")
        # -0.0 slopes are 0.0 slopes
        a, b = K.random_lines(A, 6000 + A)
        b[::2] = 0.0
        bz = b.copy()
        bz[::4] = -0.0
        kg, _, _ = check_columns(h, a, bz, "-0.0 slopes")
        assert kg[0] == envelope(h, a, b)[0][0]
        # breakpoints beyond |z| = 40: no NaN, and where the reference underflows a value as small
        b = np.linspace(0.0, 1.0, A)
        a = -b * (41.0 + np.arange(A) / A)
        kg, _ = envelope(h, a, np.stack([b, -b], axis=1))
        ref = np.array([R.ref_h(a, b), R.ref_h(a, -b)])
        assert np.all(np.isfinite(kg)) and np.all(ref < 1e-280) and np.all(kg >= 0) and np.all(kg <= 1e-279)
        check_columns(h, *K.far(34.7), "far")
    # dyadic a shifted by 2^20: bitwise the unshifted result (a enters as differences only)
    a, b = K.grid(A, 7000 + A)
    kg, nseg = envelope(h, a, b)
    kg2, nseg2 = envelope(h, a + 2.0 ** 20, b)
    assert np.array_equal(kg, kg2) and np.array_equal(nseg, nseg2)


def test_envelope_status(any_handle, engine_lib):
    h = any_handle
    a = np.zeros(2049)
    assert h.kg_envelope(a, np.zeros((2049, 1)), check=False)[0] == -1, "A = 2049 is GPE_ERR_ARG"
    raw = engine_lib.fn("kg_envelope")
    a, B, kg = np.zeros(8), np.zeros((8, 2), order="F"), np.full(2, -7.0)
    assert raw(h._h, _capi._d(a), 8, _capi._d(B), 7, 2, _capi._d(kg), None) == -1, "ldb < A"
    assert raw(h._h, _capi._d(a), 0, _capi._d(B), 8, 2, _capi._d(kg), None) == -1, "A < 1"
    assert raw(h._h, _capi._d(a), 8, _capi._d(B), 8, -1, _capi._d(kg), None) == -1, "M < 0"
    assert raw(h._h, _capi._d(a), 8, _capi._d(B), 8, 0, _capi._d(kg), None) == 0 and np.all(kg == -7.0), "M = 0 is a no-op"
    assert raw(h._h, _capi._d(a), 8, _capi._d(B), 8, 2, _capi._d(kg), None) == 0 and np.all(kg == 0.0), "nseg may be NULL"
    # NaN and inf inputs: the walk is bounded, the call returns
    a = np.array([0.0, np.nan, 1.0, np.inf, -np.inf, 2.0])
    b = np.array([np.nan, 0.5, np.inf, -1.0, 1.0, -np.inf])
    rc, _, nseg = h.kg_envelope(a, b.reshape(6, 1))
    assert rc == 0 and 0 <= nseg[0] <= 6


# ------------------------------------------------------------------------------------------------ 2. and 3. the call
def get_problem(name, oracle_lib):
    if name == "matern52_40x129":
        pr = dict(small_problem(oracle_lib, 40, 129))
        pr.update(N=40, M=129, D=6, P=1)
        return pr
    return problem(name, oracle_lib)


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_inputs_against_the_oracle(engine_lib, oracle_lib, name):
    pr = get_problem(name, oracle_lib)
    A = PROBLEMS[name]
    h = model(engine_lib, pr)
    Va, Vc, Sig = pr["V"][:A], pr["V"][A:], pr["Sig"]
    rc, kg, var, cov = h.kg_batch(Va, Vc, NOISE)
    assert rc == 0
    _, v0 = h.query_batch(Vc)
    d_cov, d_var, d_v0 = np.max(np.abs(cov - Sig[:A, A:])), np.max(np.abs(var - np.diag(Sig)[A:])), np.max(np.abs(var - v0))
    print(f"max|cov - ref| = {d_cov:.3e}, max|var_c - ref| = {d_var:.3e}, max|var_c - query_batch| = {d_v0:.3e}")
    assert d_cov <= 1e-8 and d_var <= 1e-8 and d_v0 <= 1e-10
    assert h.flow_retries() == 0 and h.handover_reruns() == 0
    h.close()


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_call_against_the_reference_envelope(engine_lib, oracle_lib, name):
    """the reference envelope fed the device's own cov and var_c and the means passed in"""
    pr = get_problem(name, oracle_lib)
    A = PROBLEMS[name]
    h = model(engine_lib, pr)
    Va, Vc = pr["V"][:A], pr["V"][A:]
    M = len(Vc)
    mu = pr["kta"][:, 0].copy()  # complete means, as a caller with a mean functor would pass them
    ka, _ = h.query_batch(Va)
    kc, _ = h.query_batch(Vc)
    for with_self in (False, True):
        for lam in (NOISE, 0.0):
            rc, kg, var, cov = h.kg_batch(Va, Vc, lam, with_self, mu_a=mu[:A], mu_c=mu[A:])
            assert rc == 0
            ref = np.array([R.ref_kg_column(mu[:A], cov[:, m], var[m], mu[A + m], lam, with_self) for m in range(M)])
            e = rel_err(kg, ref)
            print(f"with_self {int(with_self)} lambda {lam}: kg in [{ref.min():.3e}, {ref.max():.3e}], median {np.median(ref):.3e}, "
                  f"max relative error {e:.3e}")
            assert e <= BAR
            # no means passed: bitwise the call with gpe_query_batch's kta of output 0 passed
            r0 = h.kg_batch(Va, Vc, lam, with_self)
            r1 = h.kg_batch(Va, Vc, lam, with_self, mu_a=ka[:, 0], mu_c=kc[:, 0])
            assert r0[0] == r1[0] == 0 and all(np.array_equal(x, y) for x, y in zip(r0[1:], r1[1:]))
            ref0 = np.array([R.ref_kg_column(ka[:, 0], r0[3][:, m], r0[2][m], kc[m, 0], lam, with_self) for m in range(M)])
            assert rel_err(r0[1], ref0) <= BAR
            assert np.array_equal(r0[2], var) and np.array_equal(r0[3], cov), "var_c and cov do not depend on the means"
    assert h.flow_retries() == 0 and h.handover_reruns() == 0
    h.close()


# ------------------------------------------------------------------------------------------------ 4. end to end
LAM4 = 0.1
_e2e = {}


def e2e_problem(oracle_lib):
    """N = 300, D = 6, SE-ARD with ELL6, kernel noise 0.1, y = sin(3 x.w) + 0.3 eps - mean, default_rng(1), 128 random alternatives
    and 200 random candidates: a noisy, data-poor problem on which the knowledge gradient is large"""
    if not _e2e:
        rng = np.random.default_rng(1)
        N, D, A, M = 300, 6, 128, 200
        X = rng.random((N, D))
        w = rng.random(D)
        y = np.sin(3.0 * X @ w) + 0.3 * rng.standard_normal(N)
        Va, Vc = rng.random((A, D)), rng.random((M, D))
        Sig, mu = dropin_reference(oracle_lib, O.SE_ARD, 0, X, y.reshape(N, 1), np.vstack([Va, Vc]), LAM4, th=ELL6)
        ref = {ws: R.ref_kg(Sig, mu[:, 0], np.arange(A), A + np.arange(M), LAM4, bool(ws)) for ws in (0, 1)}
        _e2e.update(X=X, y=y, om=(y - y.mean()).reshape(N, 1), Va=Va, Vc=Vc, ref=ref, A=A, M=M)
    return _e2e


def e2e_preconditions(ref):
    """on the reference alone — conditions on the inputs, not skips"""
    s = np.sort(ref)[::-1]
    assert s[0] >= 1e-3 and np.mean(ref >= 1e-4) >= 0.10 and (s[0] - s[1]) / s[0] >= 1e-4, (s[0], np.mean(ref >= 1e-4), (s[0] - s[1]) / s[0])


E2E_BOUND = 2e-8 + 0.8e-8 * (LAM4 ** -0.5 + 1.0 / (3.0 * math.sqrt(3.0) * LAM4))  # 6.07e-8


@pytest.mark.parametrize("with_self", [0, 1])
def test_end_to_end(engine_lib, oracle_lib, with_self):
    pr = e2e_problem(oracle_lib)
    ref = pr["ref"][with_self]
    e2e_preconditions(ref)
    h = _capi.Handle(engine_lib)
    h.set_data(pr["X"], pr["om"])
    h.set_kernel(O.SE_ARD, ELL6, LAM4)
    assert h.compute() == 0
    rc, kg, _, _ = h.kg_batch(pr["Va"], pr["Vc"], LAM4, bool(with_self))
    d = np.max(np.abs(kg - ref))
    print(f"with_self {with_self}: max kg {ref.max():.3e}, share >= 1e-4 {np.mean(ref >= 1e-4):.2f}, max|kg - ref| = {d:.3e} (bound {E2E_BOUND:.3e})")
    assert rc == 0 and int(np.argmax(kg)) == int(np.argmax(ref))
    assert d <= E2E_BOUND
    h.close()


# ------------------------------------------------------------------------------------------------ 5. determinism and constness
@pytest.mark.parametrize("name", ["se_ard_300x65_p2", "matern52_40x129", "matern52_1700x700"])
def test_determinism_and_constness(engine_lib, oracle_lib, name):
    pr = get_problem(name, oracle_lib)
    A = PROBLEMS[name]
    h = model(engine_lib, pr)
    Va, Vc = pr["V"][:A], pr["V"][A:]
    M = len(Vc)
    ep0, ll0 = h.epoch(), h.log_lik()
    k0, v0 = h.query_batch(pr["V"])
    a = h.kg_batch(Va, Vc, NOISE, True)
    b = h.kg_batch(Va, Vc, NOISE, True)
    assert a[0] == b[0] == 0 and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), "two calls are bitwise equal in every output"
    half = M // 2
    lo, hi = h.kg_batch(Va, Vc[:half], NOISE, True), h.kg_batch(Va, Vc[half:], NOISE, True)
    for k in (1, 2, 3):
        assert np.array_equal(np.concatenate([lo[k], hi[k]], axis=-1), a[k]), "two halves are bitwise the batch"
    for m in range(M):
        one = h.kg_batch(Va, Vc[m:m + 1], NOISE, True)
        assert one[1][0] == a[1][m] and one[2][0] == a[2][m] and np.array_equal(one[3][:, 0], a[3][:, m]), f"candidate {m} alone"
    assert h.epoch() == ep0 and h.log_lik() == ll0
    k1, v1 = h.query_batch(pr["V"])
    assert np.array_equal(k0, k1) and np.array_equal(v0, v1), "gpe_query_batch answers bitwise what it answered before"
    assert h.flow_retries() == 0 and h.handover_reruns() == 0
    h.close()


def test_status_and_phases(engine_lib, oracle_lib):
    pr = problem("se_ard_300x65_p2", oracle_lib)
    A = 33
    Va, Vc = pr["V"][:A], pr["V"][A:]
    h = _capi.Handle(engine_lib)
    h.set_data(pr["X"], pr["om"])
    h.set_kernel(pr["kind"], pr["th"], NOISE)
    call = lambda Xa=Va, Xc=Vc, lam=NOISE, **kw: h.kg_batch(Xa, Xc, lam, check=False, **kw)[0]
    assert call() == -2, "GPE_ERR_STATE before compute"
    assert h.kg_envelope(np.zeros(3), np.ones((3, 1)))[0] == 0, "the envelope alone needs no computed model"
    assert h.compute() == 0
    assert call() == 0
    for bad in (-1e-9, float("nan"), float("inf")):
        assert call(lam=bad) == -1
    assert call(Xa=np.zeros((2049, pr["D"]))) == -1, "A > 2048"
    raw = engine_lib.fn("kg_batch")
    Xa, Xc = np.ascontiguousarray(Va), np.ascontiguousarray(Vc)
    kg = np.full(len(Vc), -7.0)
    cov = np.zeros((A, len(Vc)), order="F")
    assert raw(h._h, _capi._d(Xa), 0, None, _capi._d(Xc), len(Vc), None, NOISE, 0, _capi._d(kg), None, None, 0) == -1, "A < 1"
    assert raw(h._h, _capi._d(Xa), A, None, _capi._d(Xc), -1, None, NOISE, 0, _capi._d(kg), None, None, 0) == -1, "M < 0"
    assert raw(h._h, _capi._d(Xa), A, None, _capi._d(Xc), len(Vc), None, NOISE, 0, None, None, _capi._d(cov), A - 1) == -1, "ldc < A"
    assert raw(h._h, _capi._d(Xa), A, None, _capi._d(Xc), 0, None, NOISE, 0, _capi._d(kg), None, None, 0) == 0 and np.all(kg == -7.0), "M = 0"
    # NULL outputs in every combination: what is asked for is bitwise what the full call gives
    names = ("kg", "var", "cov")
    full = h.kg_batch(Va, Vc, NOISE, True)
    for mask in range(8):
        want = tuple(n for k, n in enumerate(names) if mask >> k & 1)
        got = h.kg_batch(Va, Vc, NOISE, True, want=want)
        assert got[0] == 0
        for k, n in enumerate(names):
            assert (got[1 + k] is None) if n not in want else np.array_equal(got[1 + k], full[1 + k])
    h.set_profiling(True)
    assert h.kg_batch(Va, Vc, NOISE, True)[0] == 0
    ms = h.kg_phase_ms()
    print(ms)
    assert set(ms) == {"alternatives", "candidates", "envelope", "readback"}
    assert ms["alternatives"] > 0 and ms["candidates"] > 0 and ms["envelope"] > 0 and ms["readback"] >= 0
    h.close()
    k = _capi.Handle(engine_lib)
    Xs = pr["X"][:300]
    k.set_data(Xs, pr["om"][:300])
    k.set_kernel(_capi.KERNEL_HOST_K, np.zeros(0), NOISE)
    k.set_K_host(O.kernel_matrix(pr["kind"], Xs, pr["th"], NOISE))
    assert k.compute() == 0
    assert k.kg_batch(Va, Vc, NOISE, check=False)[0] == -5, "GPE_ERR_UNSUPPORTED for GPE_KERNEL_HOST_K"
    assert k.kg_envelope(np.zeros(3), np.ones((3, 1)), check=False)[0] == -5
    k.close()


# ------------------------------------------------------------------------------------------------ 6. the C++ drop-in on the device
@pytest.mark.parametrize("with_self", [0, 1])
def test_dropin_on_the_device(tmp_path, oracle_lib, with_self):
    """kg_best at N = 300 (above Params::gpu::min_n_for_gpu: through gpe_kg_batch) is the reference's arg-max on the problem of the
    end-to-end test"""
    pr = e2e_problem(oracle_lib)
    ref = pr["ref"][with_self]
    e2e_preconditions(ref)
    got = run_driver(tmp_path, 0, 0, pr["X"], pr["y"].reshape(-1, 1), pr["Va"], pr["Vc"], 0, with_self, noise_id=1, hp=ELL6)
    assert got["host_resident"][0] == 0
    assert int(got["best"][0]) == int(np.argmax(ref))
    assert np.max(np.abs(got["kg"] - ref)) <= E2E_BOUND


@pytest.mark.parametrize("n", [255, 257])
def test_dropin_host_and_device_agree(tmp_path, oracle_lib, n):
    """n on either side of Params::gpu::min_n_for_gpu (256), each forced through both paths: the same numbers within the bound of
    the end-to-end test, and both the reference's"""
    pr = e2e_problem(oracle_lib)
    X, y = pr["X"][:n], pr["y"][:n].reshape(-1, 1)
    Va, Vc = pr["Va"][:64], pr["Vc"][:64]
    host = run_driver(tmp_path, 0, 0, X, y, Va, Vc, 0, 1, noise_id=1, hp=ELL6,
                      env={"LIMBO_AMD_MIN_N_FOR_GPU": str(1 << 20), "LIMBO_AMD_HOST_BATCH_CROSSOVER": str(1 << 40)})
    dev = run_driver(tmp_path, 0, 0, X, y, Va, Vc, 0, 1, noise_id=1, hp=ELL6, env={"LIMBO_AMD_MIN_N_FOR_GPU": "0"})
    nat = run_driver(tmp_path, 0, 0, X, y, Va, Vc, 0, 1, noise_id=1, hp=ELL6)
    assert host["host_resident"][0] == 1 and dev["host_resident"][0] == 0 and nat["host_resident"][0] == (1 if n < 256 else 0)
    Sig, mu = dropin_reference(oracle_lib, O.SE_ARD, 0, X, y, np.vstack([Va, Vc]), LAM4, th=ELL6)
    ref = R.ref_kg(Sig, mu[:, 0], np.arange(64), 64 + np.arange(64), LAM4, True)
    assert ref.max() >= 1e-3
    for got in (host, dev, nat):
        assert np.max(np.abs(got["kg"] - ref)) <= E2E_BOUND and int(got["best"][0]) == int(np.argmax(ref))
    assert np.max(np.abs(host["kg"] - dev["kg"])) <= E2E_BOUND


# ------------------------------------------------------------------------------------------------ the fused calls' second chunk
CHUNK_NM = 8192  # candidates per chunk of a fused call in the N x M layout (fewer samples than one outer panel)


def two_chunk_model(engine_lib, P):
    """N = 200 samples (the N x M layout), D = 4, P outputs, SE-ARD; CHUNK_NM + 65 candidates: a fused call runs its loop twice"""
    rng = np.random.default_rng(8192 + P)
    N, D, M = 200, 4, CHUNK_NM + 65
    X = rng.random((N, D))
    Y = np.stack([np.sin(3.0 * X @ rng.random(D)) for _ in range(P)], axis=1) + 0.1 * rng.standard_normal((N, P))
    h = _capi.Handle(engine_lib)
    h.set_data(X, Y - Y.mean(axis=0))
    h.set_kernel(O.SE_ARD, np.log([0.3, 0.5, 0.7, 0.9, 1.0]), 0.1)
    assert h.compute() == 0
    return h, rng.random((M, D)), rng


def check_second_chunk(call, M):
    """call(sel): every returned array of the fused call on the candidates V[sel] (with their rows of mean_add), candidates along
    axis 0.  The whole batch's answers behind the chunk boundary are bitwise those of the same candidates asked alone, and so are
    the candidates on either side of the boundary."""
    assert M > CHUNK_NM
    whole = call(slice(0, M))
    assert all(w.shape[0] == M and not np.any(np.isnan(w)) for w in whole)
    tail = call(slice(CHUNK_NM, M))
    for w, t in zip(whole, tail):
        assert np.array_equal(w[CHUNK_NM:], t), "the second chunk's candidates asked alone"
    for m in (CHUNK_NM - 1, CHUNK_NM):
        for w, o in zip(whole, call(slice(m, m + 1))):
            assert np.array_equal(w[m:m + 1], o), f"candidate {m} alone"


def test_fused_second_chunk(engine_lib):
    h, V, rng = two_chunk_model(engine_lib, 1)
    Xa, mu_c = rng.random((65, V.shape[1])), 0.05 * rng.standard_normal(len(V))

    def call(sel):
        rc, kg, var, cov = h.kg_batch(Xa, V[sel], 0.1, with_self=True, mu_c=mu_c[sel])
        assert rc == 0
        return kg, var, cov.T

    check_second_chunk(call, len(V))
    assert np.any(call(slice(CHUNK_NM, len(V)))[0] > 0)
    h.close()
