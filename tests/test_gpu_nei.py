"""Noisy expected improvement in the log domain on the device (include/gpe_nei.h).

The checker is never the engine: tests/nei_ref.py's numpy / scipy ref_lognei, whose own error against 50-digit arithmetic is E_REF_NEI
(tests/test_nei_host.py), and ref_pipeline, the whole call from LAPACK factors.  The measure is |got - ref| / max(1, |ref|).  Bars:
* the kernel given equal conditional beliefs: BAR = 16 E_REF_NEI, value and every term;
* the fused call's mu and var against gpe_query_batch: 1e-10;
* fplus, cmean and cvar against ref_pipeline: the project's parity bar, 1e-8;
* lognei end to end: 10 E_REF_NEI max(1, |ref|) + max_s |d term_s / d m| 1e-8 + max_s |d term_s / d sd| 1e-8 / (2 sd) — the 1e-8 bar on
  cmean and cvar pushed through to first order (the weights of the log-mean-exp sum to 1), over candidates with every |z_s| <= 10 and
  cvar >= 1e-4.  Derived, not measured; that at least half of the candidates qualify is asserted on the reference alone."""
import numpy as np
import pytest

from limbo_amd import _capi
from oracle import np_oracle as O
from tests import nei_ref as R
from tests.test_nei_host import BAR, E_REF_NEI

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
NOISE, JITTER, XI = 0.01, 1e-6, 0.01
ELL = np.log([0.5] * 6 + [1.0])  # SE-ARD, D = 6, isotropic length scale 0.5, sigma_f = 1
ELL_1700 = np.log([0.35] * 6 + [1.0])  # ... 0.35 for 1700 samples: with 0.5 their posterior variance leaves 0.36 of the candidates qualifying
AMP = 0.3  # the objective's amplitude over observation noise 0.1: with 1.0 the means lie up to 30 conditional sd below the incumbents


@pytest.fixture(scope="module")
def any_handle(engine_lib):
    h = _capi.Handle(engine_lib)  # (not computed, no data: the kernel alone needs the device only)
    yield h
    h.close()


def random_beliefs(S, M, rng):
    """z in [-30, 6]; four candidates in ten are mild (every z in [-2, 6]) so that their lognei is above -20"""
    mild = rng.random(M) < 0.4
    z = np.where(mild[None, :], rng.uniform(-2, 6, (S, M)), rng.uniform(-30, 6, (S, M)))
    sd = 10 ** rng.uniform(-1.3, 0.7, M)
    fplus = rng.uniform(0.3, 0.5, S)
    return dict(fplus=fplus, xi=XI, cmean=np.asfortranarray(fplus[:, None] + XI + z * sd[None, :]), sd=sd)


def ref_of(b):
    return R.ref_lognei(b["fplus"], b["xi"], b["cmean"], b["sd"])


def dev_of(h, b, cols=slice(None), **kw):
    rc, v, t = h.lognei_values(b["fplus"], np.asfortranarray(b["cmean"][:, cols]), b["sd"][cols], b["xi"], **kw)
    assert rc == 0
    return v, t


def errors(got, ref):
    return [float(R.err(g, r).max()) if np.size(r) else 0.0 for g, r in zip(got, ref)]


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
@pytest.mark.parametrize("M", [1, 63, 65, 257])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 257, 1024])
def test_values_random(any_handle, S, M):
    b = random_beliefs(S, M, np.random.default_rng(1000 * S + M))
    got, ref = dev_of(any_handle, b), ref_of(b)
    ev, et = errors(got, ref)
    print(f"S = {S}, M = {M}: lognei in [{ref[0].min():.3e}, {ref[0].max():.3e}]; error: value {ev:.3e}, terms {et:.3e} (BAR {BAR:.3e})")
    assert max(ev, et) <= BAR
    if M >= 63:
        assert np.mean(ref[0] > -20) >= 0.2 and np.mean(got[0] > -20) >= 0.2, "a kernel that returns -inf must not pass"
    again = dev_of(any_handle, b)
    assert all(np.array_equal(x, y) for x, y in zip(got, again)), "two calls are bitwise equal"
    v, t = dev_of(any_handle, b, want=())
    assert np.array_equal(v, got[0]) and t is None
    for m in sorted({0, M // 2, M - 1}):
        one = dev_of(any_handle, b, cols=slice(m, m + 1))
        assert np.array_equal(one[0], got[0][m:m + 1]) and np.array_equal(one[1], got[1][:, m:m + 1]), f"candidate {m} alone"


def test_values_across_the_chunk(any_handle):
    """16 384 + 3 candidates: the second chunk of gpe_lognei_values"""
    S, M = 65, 16384 + 3
    b = random_beliefs(S, M, np.random.default_rng(5))
    got, ref = dev_of(any_handle, b), ref_of(b)
    ev, et = errors(got, ref)
    print(f"M = {M}: error: value {ev:.3e}, terms {et:.3e}")
    assert max(ev, et) <= BAR and np.mean(got[0] > -20) >= 0.2
    tail = dev_of(any_handle, b, cols=slice(16384, None))
    assert np.array_equal(got[0][16384:], tail[0]) and np.array_equal(got[1][:, 16384:], tail[1]), "the second chunk's candidates, asked alone"


def test_values_padding_is_not_read(any_handle):
    """ldm > S with NaN behind row S of every column"""
    S, M, pad = 65, 70, 7
    b = random_beliefs(S, M, np.random.default_rng(6))
    wide = np.full((S + pad, M), np.nan, order="F")
    wide[:S] = b["cmean"]
    rc, v, t = any_handle.lognei_values(b["fplus"], wide[:S], b["sd"], b["xi"])
    assert rc == 0 and wide[:S].strides == (8, 8 * (S + pad))
    base = dev_of(any_handle, b)
    assert np.array_equal(v, base[0]) and np.array_equal(t, base[1]) and not np.any(np.isnan(v))


def test_values_special_inputs(any_handle):
    h = any_handle
    S, M = 65, 24
    b = random_beliefs(S, M, np.random.default_rng(31))
    b["fplus"] = np.round(b["fplus"] * 64) / 64  # (exact in binary, with xi = 0.25: cmean - fplus - xi below is the offset written)
    b["xi"] = 0.25
    b["cmean"] = np.asfortranarray(b["cmean"] - XI + 0.25)
    base = dev_of(h, b)
    c = {k: np.copy(v, order="F") if isinstance(v, np.ndarray) else v for k, v in b.items()}
    # sd = 0: the improvement itself where there is one, none elsewhere; all none: -inf
    c["sd"][:2] = 0.0
    off = np.where(np.arange(S) % 3 == 0, 0.5, np.where(np.arange(S) % 3 == 1, -0.5, 0.0))
    c["cmean"][:, 0] = c["fplus"] + c["xi"] + off
    c["cmean"][:, 1] = c["fplus"] + c["xi"] - 1.0
    # -inf in every sample; +inf in one; NaN in one mean; NaN sd
    c["cmean"][:, 2] = -np.inf
    c["cmean"][7, 3] = np.inf
    c["cmean"][64, 4] = np.nan
    c["sd"][5] = np.nan
    # z = -1e8 and 1e100 standard deviations below: finite
    c["cmean"][:, 6] = c["fplus"] + c["xi"] - 1e8 * c["sd"][6]
    c["cmean"][:, 7] = -1e100 * c["sd"][7]
    v, t = dev_of(h, c)
    rv, rt = ref_of(c)
    n_pos = int(np.sum(off > 0))
    assert np.all(t[off > 0, 0] == np.log(0.5)) and np.all(t[off <= 0, 0] == -np.inf)
    assert abs(v[0] - np.log(0.5 * n_pos / S)) <= 1e-14
    assert v[1] == -np.inf and np.all(t[:, 1] == -np.inf), "sd = 0 and no improvement anywhere"
    assert v[2] == -np.inf and np.all(t[:, 2] == -np.inf)
    assert v[3] == np.inf and t[7, 3] == np.inf and not np.any(np.isnan(t[:, 3])), "a mean of +inf: +inf, never NaN"
    assert np.isnan(v[4]) and np.all(np.isnan(t[:, 4])) and np.isnan(v[5]) and np.all(np.isnan(t[:, 5])), "NaN for that candidate"
    assert np.isfinite(v[6]) and v[6] < -4e15 and np.isfinite(v[7]) and v[7] < -1e199
    fin = [0, 6, 7]
    assert max(errors((v[fin], t[:, [6, 7]]), (rv[fin], rt[:, [6, 7]]))) <= BAR
    assert np.array_equal(v[8:], base[0][8:]) and np.array_equal(t[:, 8:], base[1][:, 8:]), "the others are untouched"


# ------------------------------------------------------------------------------------------------ the model problems
# name: (kind, N, B, S, M, P, out, log theta, with the mean functor's values)
CASES = {
    "se_ard_300_b65_s64_m700": (O.SE_ARD, 300, 65, 64, 700, 1, 0, ELL, False),
    "se_ard_300_b130_s65_m70": (O.SE_ARD, 300, 130, 65, 70, 1, 0, ELL, False),
    "se_ard_200_b33_s64_m70": (O.SE_ARD, 200, 33, 64, 70, 1, 0, ELL, False),  # the N x M layout: below one outer panel
    "se_ard_300_b1_s1_m70": (O.SE_ARD, 300, 1, 1, 70, 1, 0, ELL, False),
    "matern52_300_b65_s64_m70_p2": (O.MATERN52, 300, 65, 64, 70, 2, 1, np.log([0.7, 1.0]), True),
    "se_ard_1700_b300_s64_m70": (O.SE_ARD, 1700, 300, 64, 70, 1, 0, ELL_1700, False),  # the baseline's own order crosses 256
}
_cache = {}


def problem(name):
    """inputs and ref_pipeline's numbers of a case (once per session).  The baseline: the B best observed points."""
    if name in _cache:
        return _cache[name]
    kind, N, B, S, M, P, out, th, means = CASES[name]
    rng = np.random.default_rng(100 + list(CASES).index(name))
    D = 6
    X, V = rng.random((N, D)), rng.random((M, D))
    Y = np.stack([AMP * np.sin(3.0 * X @ rng.random(D)) + 0.1 * rng.standard_normal(N) for _ in range(P)], axis=1)
    om = Y - Y.mean(axis=0)
    Xb = X[np.argsort(-om[:, out], kind="stable")[:B]]
    Z = np.asfortranarray(rng.standard_normal((B, S)))
    mean_b = np.full(B, Y.mean(axis=0)[out]) if means else None
    mean_add = (Y.mean(axis=0)[out] + 0.05 * rng.standard_normal(M)) if means else None
    ref = R.ref_pipeline(kind, th, NOISE, X, om, out, Xb, mean_b, JITTER, Z, XI, V, mean_add)
    pr = dict(kind=kind, N=N, B=B, S=S, M=M, P=P, D=D, out=out, th=th, X=X, V=V, om=om, Xb=Xb, Z=Z, mean_b=mean_b, mean_add=mean_add, ref=ref)
    _cache[name] = pr
    return pr


def model(engine_lib, pr):
    h = _capi.Handle(engine_lib)
    h.set_data(pr["X"], pr["om"])
    h.set_kernel(pr["kind"], pr["th"], NOISE)
    assert h.compute() == 0
    return h


def call(h, pr, V=None, mean_add=None, **kw):
    V = pr["V"] if V is None else V
    kw.setdefault("jitter", JITTER)
    kw.setdefault("xi", XI)
    return h.lognei_batch(V, kw.pop("Xb", pr["Xb"]), kw.pop("Z", pr["Z"]), pr["out"], mean_b=pr["mean_b"],
                          mean_add=pr["mean_add"] if mean_add is None else mean_add, **kw)


def qualifying(ref):
    """candidates the end-to-end bound speaks about: every |z_s| <= 10 and cvar >= 1e-4"""
    with np.errstate(all="ignore"):
        z = (ref["cmean"] - ref["fplus"][:, None] - XI) / ref["sd"][None, :]
    return (ref["cvar"] >= 1e-4) & np.all(np.abs(z) <= 10, axis=0)


def e2e_bound(pr):
    ref = pr["ref"]
    dm, ds = R.term_partials(ref["fplus"], XI, ref["cmean"], ref["sd"])
    with np.errstate(all="ignore"):
        return (10 * E_REF_NEI * np.maximum(1.0, np.abs(ref["lognei"])) + np.abs(dm).max(axis=0) * 1e-8
                + np.abs(ds).max(axis=0) * 1e-8 / (2.0 * ref["sd"]))


@pytest.mark.parametrize("name", list(CASES))
def test_e2e_preconditions(name):
    """on the reference alone: at least half of the candidates qualify, the baseline's covariance is well conditioned, and the plain
    value is 0 somewhere or the values are spread — the log domain is exercised"""
    pr = problem(name)
    ref = pr["ref"]
    keep = qualifying(ref)
    print(f"{name}: {keep.mean():.2f} qualify; cond(Sigma_b) = {ref['cond']:.3g}; lognei in [{np.nanmin(ref['lognei']):.3e}, "
          f"{np.nanmax(ref['lognei']):.3e}]; cvar in [{ref['cvar'].min():.3e}, {ref['cvar'].max():.3e}]")
    assert keep.mean() >= 0.5
    assert ref["cond"] <= 1e4, "fplus, cmean and cvar are comparable at 1e-8"
    assert np.all(np.isfinite(ref["lognei"]))


# ------------------------------------------------------------------------------------------------ 2. metamorphic
def test_zero_normals_is_plain_log_ei(engine_lib, any_handle):
    """Z = 0: every draw is the mean, fplus = max mu_b and cmean = mu, so lognei = gpe_logcei_values' log EI on (mu, sqrt(clamped cvar))"""
    pr = problem("se_ard_300_b65_s64_m700")
    h = model(engine_lib, pr)
    rc, ln, fplus, mu, var, cvar, cmean = call(h, pr, Z=np.zeros_like(pr["Z"]))
    assert rc == 0
    assert np.all(fplus == fplus[0]) and np.all(cmean == mu[None, :]), "every draw is the mean"
    kb, _ = h.query_batch(pr["Xb"])
    assert abs(fplus[0] - kb[:, 0].max()) <= 1e-10
    sd = np.sqrt(np.where(cvar > EPS, cvar, 0.0))
    rc, lc, _, _ = any_handle.logcei_values(np.zeros(0), np.zeros((pr["M"], 0)), np.zeros((pr["M"], 0)), mu, sd, float(fplus[0]), XI, True, want=())
    e = float(R.err(ln, lc).max())
    print(f"Z = 0: lognei in [{ln.min():.3e}, {ln.max():.3e}], against gpe_logcei_values {e:.3e}")
    assert rc == 0 and e <= BAR and np.all(np.isfinite(ln))
    h.close()


# ------------------------------------------------------------------------------------------------ 3. the pipeline
@pytest.mark.parametrize("name", list(CASES))
def test_pipeline(engine_lib, any_handle, name):
    pr = problem(name)
    ref = pr["ref"]
    h = model(engine_lib, pr)
    k0, v0 = h.query_batch(pr["V"])
    rc, ln, fplus, mu, var, cvar, cmean = call(h, pr)
    assert rc == 0
    want_mu = k0[:, pr["out"]] + (0.0 if pr["mean_add"] is None else pr["mean_add"])
    d_mu, d_var = np.max(np.abs(mu - want_mu)), np.max(np.abs(var - v0))
    e_f, e_m, e_v = (float(R.err(g, ref[k]).max()) for g, k in ((fplus, "fplus"), (cmean, "cmean"), (cvar, "cvar")))
    keep = qualifying(ref)
    bound = e2e_bound(pr)
    d = np.abs(ln - ref["lognei"])
    # the kernel on the device's own conditional beliefs
    sd = np.sqrt(np.where(cvar > EPS, cvar, 0.0))
    rv, _ = R.ref_lognei(fplus, XI, cmean, sd)
    e_k = float(R.err(ln, rv).max())
    print(f"{name}: max|mu - query| {d_mu:.3e}, max|var - query| {d_var:.3e}; fplus {e_f:.3e}, cmean {e_m:.3e}, cvar {e_v:.3e}; "
          f"lognei: kernel on its own beliefs {e_k:.3e}, end to end max {d[keep].max():.3e}, worst share of the bound "
          f"{np.max(d[keep] / bound[keep]):.3e} over {keep.sum()} of {pr['M']}")
    assert d_mu <= 1e-10 and d_var <= 1e-10
    assert max(e_f, e_m, e_v) <= 1e-8
    assert e_k <= BAR
    assert np.all(d[keep] <= bound[keep]) and np.all(np.isfinite(ln))
    assert np.all(cvar <= var + 1e-12), "conditioning never adds variance"
    assert h.flow_retries() == 0 and h.handover_reruns() == 0
    h.close()


# ------------------------------------------------------------------------------------------------ 4. bitwise
@pytest.mark.parametrize("name", ["se_ard_300_b65_s64_m700", "se_ard_200_b33_s64_m70", "se_ard_1700_b300_s64_m70"])
def test_batch_invariance(engine_lib, name):
    pr = problem(name)
    h = model(engine_lib, pr)
    M = pr["M"]
    full = call(h, pr)
    again = call(h, pr)
    assert all(np.array_equal(x, y) for x, y in zip(full[1:], again[1:])), "the same call twice"
    cut = M // 2 | 1
    ma = pr["mean_add"]
    lo = call(h, pr, V=pr["V"][:cut], mean_add=None if ma is None else ma[:cut])
    hi = call(h, pr, V=pr["V"][cut:], mean_add=None if ma is None else ma[cut:])
    for k in (1, 3, 4, 5):
        assert np.array_equal(np.concatenate([lo[k], hi[k]]), full[k]), "two parts are bitwise the batch"
    assert np.array_equal(np.concatenate([lo[6], hi[6]], axis=1), full[6]) and np.array_equal(lo[2], full[2])
    for m in (0, 7, M - 1):
        one = call(h, pr, V=pr["V"][m:m + 1], mean_add=None if ma is None else ma[m:m + 1])
        assert one[1][0] == full[1][m] and one[5][0] == full[5][m] and np.array_equal(one[6][:, 0], full[6][:, m]), f"candidate {m} alone"
    h.close()


def test_across_the_chunk_boundary(engine_lib):
    """M = 16 384 + 70 at N = 300: the second chunk's candidates, asked alone"""
    pr = problem("se_ard_300_b65_s64_m700")
    h = model(engine_lib, pr)
    V = np.random.default_rng(9).random((16384 + 70, pr["D"]))
    V[16384:] = pr["V"][:70]
    big = call(h, pr, V=V, want=("lognei", "cvar", "cmean"))
    tail = call(h, pr, V=V[16384:], want=("lognei", "cvar", "cmean"))
    small = call(h, pr, V=pr["V"][:70], want=("lognei", "cvar", "cmean"))
    assert big[0] == 0 and np.all(np.isfinite(big[1]))
    for a in (tail, small):
        assert np.array_equal(big[1][16384:], a[1]) and np.array_equal(big[5][16384:], a[5]) and np.array_equal(big[6][:, 16384:], a[6])
    h.close()


# ------------------------------------------------------------------------------------------------ 5. the model is not changed
def test_model_is_not_changed(engine_lib):
    pr = problem("se_ard_300_b130_s65_m70")
    h = model(engine_lib, pr)
    ep0 = h.epoch()
    Zd = np.random.default_rng(4).standard_normal((pr["M"], 8, 1))
    q0 = h.query_batch(pr["V"])
    j0 = h.joint_draws(pr["V"], Zd, 1e-8)
    c0 = h.joint_query(pr["V"], 1e-8)
    assert call(h, pr)[0] == 0
    assert h.epoch() == ep0
    q1 = h.query_batch(pr["V"])
    j1 = h.joint_draws(pr["V"], Zd, 1e-8)
    c1 = h.joint_query(pr["V"], 1e-8)
    flat = lambda r: [np.asarray(x) for x in (r if isinstance(r, (tuple, list)) else (r,)) if x is not None and not np.isscalar(x)]
    for a, b in ((q0, q1), (j0, j1), (c0, c1)):
        assert len(flat(a)) == len(flat(b)) >= 1 and all(np.array_equal(x, y) for x, y in zip(flat(a), flat(b)))
    h.close()


# ------------------------------------------------------------------------------------------------ 6. statuses
def test_status_and_phases(engine_lib, any_handle):
    pr = problem("se_ard_300_b65_s64_m700")
    h = _capi.Handle(engine_lib)
    h.set_data(pr["X"], pr["om"])
    h.set_kernel(pr["kind"], pr["th"], NOISE)
    assert call(h, pr, check=False)[0] == -2, "GPE_ERR_STATE before compute"
    assert h.lognei_values([0.0], [[0.0]], [1.0])[0] == 0, "the kernel alone needs no computed model"
    assert h.compute() == 0
    ok = call(h, pr)
    assert ok[0] == 0

    def refused(out, what, rc=-1):
        assert out[0] == rc and all(np.all(x == 0.0) for x in out[1:]), what + ": nothing written"

    # Duplicated baseline points and no jitter: the covariance is singular, an ordinary status of the factorisation.  With ONE
    # duplicate the second pivot of the pair is a - fl(a / fl(sqrt(a)))^2 = 2 a (e1 - e2) in exact terms: rounding decides its sign,
    # at about even odds (tests/test_gpu_joint_posterior.py accepts 0 or the index there).  With every one of 33 points listed twice
    # the odds that no pair's pivot comes out <= 0 are 2^-33: that baseline must be refused.
    Xd = pr["Xb"].copy()
    Xd[5] = Xd[2]
    one = call(h, pr, Xb=Xd, jitter=0.0, check=False)
    print("one duplicated baseline point, jitter 0: status", one[0])
    assert one[0] in (0, 6)
    X2 = np.repeat(pr["Xb"][:33], 2, axis=0)
    Z2 = np.asfortranarray(np.random.default_rng(66).standard_normal((66, pr["S"])))
    out = call(h, pr, Xb=X2, Z=Z2, jitter=0.0, check=False)
    print("33 baseline points listed twice, jitter 0: status", out[0])
    assert 2 <= out[0] <= 66 and all(np.all(x == 0.0) for x in out[1:]), "a positive pivot status, nothing written"
    assert call(h, pr, Xb=X2, Z=Z2, jitter=1e-6)[0] == 0, "... and with jitter it is factored"
    again = call(h, pr)
    assert all(np.array_equal(x, y) for x, y in zip(ok[1:], again[1:])), "the handle serves on after a refused baseline"
    for bad in (np.inf, np.nan, -1e-9):
        refused(call(h, pr, jitter=bad, check=False), "a jitter that is negative or not finite")
    for bad in (np.inf, np.nan):
        refused(call(h, pr, xi=bad, check=False), "an xi that is not finite")
        Zb = pr["Z"].copy()
        Zb[3, 2] = bad
        refused(call(h, pr, Z=Zb, check=False), "a Z that is not finite")
    f = h.lib.fn("lognei_batch")
    d = _capi._d
    Xb, Z, V = np.ascontiguousarray(pr["Xb"]), pr["Z"], np.ascontiguousarray(pr["V"])
    val = np.zeros(pr["M"])
    raw = lambda out=0, B=pr["B"], S=pr["S"], M=pr["M"], xb=d(Xb), z=d(Z), v=d(V), cm=None, ldm=pr["S"]: f(
        h._h, out, xb, B, None, JITTER, z, S, XI, v, M, None, d(val), None, None, None, None, cm, ldm)
    assert raw() == 0 and np.array_equal(val, ok[1])
    val[:] = 0.0
    for kw, what in ((dict(out=1), "out = P"), (dict(out=-1), "out < 0"), (dict(B=0), "B = 0"), (dict(B=1025), "B = 1025"), (dict(S=0), "S = 0"),
                     (dict(S=1025), "S = 1025"), (dict(M=-1), "M < 0"), (dict(xb=None), "no baseline"), (dict(z=None), "no normals"),
                     (dict(v=None), "no candidates"), (dict(cm=d(np.zeros((pr["S"], pr["M"]), order="F")), ldm=pr["S"] - 1), "ldm < S")):
        assert raw(**kw) == -1 and np.all(val == 0.0), what
    assert raw(M=0) == 0 and np.all(val == 0.0), "M = 0 is a no-op"
    rc, v, _ = any_handle.lognei_values([0.0], [[0.0]], [-1.0], check=False)
    assert rc == -1 and v[0] == 0.0, "a negative csd"
    assert any_handle.lognei_values([np.inf], [[0.0]], [1.0], check=False)[0] == -1, "an fplus that is not finite"
    assert any_handle.lognei_values([0.0], np.zeros((1, 0)), np.zeros(0))[0] == 0, "M = 0"
    # NULL outputs: what is asked for is bitwise what the full call gives
    names = ("lognei", "fplus", "mu", "var", "cvar", "cmean")
    for mask in (1, 2, 4, 8, 16, 32, 37):
        want = tuple(n for k, n in enumerate(names) if mask >> k & 1)
        got = call(h, pr, want=want)
        for k, n in enumerate(names):
            assert (got[1 + k] is None) if n not in want else np.array_equal(got[1 + k], ok[1 + k]), (mask, n)
    h.close()
    # the phases, at a shape whose device time carries the call and whose scratch (below 64 MiB) is kept from call to call — above
    # that the handle gives it back after every call, and allocating it again is host time outside every phase: N = 1700, B = 300,
    # 1024 candidates.  Of three calls the quickest: the others' excess is the host's, not the call's.
    import time

    big = problem("se_ard_1700_b300_s64_m70")
    h = model(engine_lib, big)
    V = np.random.default_rng(12).random((1024, big["D"]))
    h.set_profiling(True)
    assert call(h, big, V=V, want=("lognei",))[0] == 0  # (the scratch is sized, the scratch context made)
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        assert call(h, big, V=V, want=("lognei",))[0] == 0
        runs.append((1e3 * (time.perf_counter() - t0), h.nei_phase_ms()))
    wall, ms = min(runs, key=lambda r: r[0])
    print([(round(w, 3), round(sum(m.values()), 3)) for w, m in runs], ms)
    assert set(ms) == {"baseline", "factor_draws", "solves", "conditioning", "kernel"} and all(v >= 0 for v in ms.values())
    assert ms["baseline"] > 0 and ms["solves"] > 0 and ms["conditioning"] > 0 and ms["kernel"] > 0
    assert 0.5 * wall <= sum(ms.values()) <= 1.05 * wall, "the phases add up to about the call"
    h.close()
    k = _capi.Handle(engine_lib)
    k.set_data(pr["X"], pr["om"])
    k.set_kernel(_capi.KERNEL_HOST_K, np.zeros(0), NOISE)
    k.set_K_host(O.kernel_matrix(pr["kind"], pr["X"], pr["th"], NOISE))
    assert k.compute() == 0
    assert call(k, pr, check=False)[0] == -5, "GPE_ERR_UNSUPPORTED for GPE_KERNEL_HOST_K"
    assert k.lognei_values([0.0], [[0.0]], [1.0], check=False)[0] == -5
    k.close()


# ------------------------------------------------------------------------------------------------ 7. the C++ drop-in on the device
from tests.test_nei_host import HOST_ENV, check_baseline, check_dropin, dropin_problem, run_driver  # noqa: E402


def test_dropin_on_the_device(tmp_path):
    """n = 600 (above Params::gpu::min_n_for_gpu: through gpe_lognei_batch, gpe_joint_draws and gpe_query_batch) against the Python
    reference's numbers; nei_baseline is a subset that holds the arg-max of the posterior mean and is deterministic for a seed;
    lognei_best picks the reference's arg-max"""
    S, seed = 16, 5
    X, Y, Q, Xb, hp = dropin_problem(600, 40, 24, 31)
    got = run_driver(tmp_path, X, Y, Q, Xb, S, seed, hp, s_prune=32)
    assert int(got["host_resident"][0]) == 0
    check_dropin(got, X, Y, Q, Xb, S, hp, "device, n = 600")
    idx = check_baseline(got, X)
    print("baseline", idx)
    assert len(idx) <= 33


def test_dropin_host_and_device_agree(tmp_path):
    """n = 255 lives on the host and n = 257 on the device by default (Params::gpu::min_n_for_gpu = 256; 14 points x 255 samples stay
    below the host's batch crossover).  Each size is then forced through BOTH paths (LIMBO_AMD_MIN_N_FOR_GPU = 0: the device; the host
    switches: the host) and the two must agree over ALL candidates: fplus, cmean and cvar within 2e-8 (each side's parity bar 1e-8),
    lognei within twice the end-to-end bound (the 1e-8 bar pushed through the terms' partials, whatever |z|)."""
    S, seed = 8, 9
    for n, host in ((255, 1), (257, 0)):
        X, Y, Q, Xb, hp = dropin_problem(n, 8, 6, 40 + n)
        got = run_driver(tmp_path, X, Y, Q, Xb, S, seed, hp)
        assert int(got["host_resident"][0]) == host, n
        check_dropin(got, X, Y, Q, Xb, S, hp, f"n = {n}, default placement")
        on_dev = run_driver(tmp_path, X, Y, Q, Xb, S, seed, hp, env={"LIMBO_AMD_MIN_N_FOR_GPU": "0"})
        on_host = run_driver(tmp_path, X, Y, Q, Xb, S, seed, hp, env=HOST_ENV)
        assert int(on_dev["host_resident"][0]) == 0 and int(on_host["host_resident"][0]) == 1
        check_dropin(on_dev, X, Y, Q, Xb, S, hp, f"n = {n} on the device")
        check_dropin(on_host, X, Y, Q, Xb, S, hp, f"n = {n} on the host")
        assert np.array_equal(on_dev["Z"], on_host["Z"])
        M, B = len(Q), len(Xb)
        fp, cm = on_host["fplus"], on_host["cmean"].reshape(M, S).T
        sd = np.sqrt(np.where(on_host["cvar"] > EPS, on_host["cvar"], 0.0))
        dm, ds = R.term_partials(fp, 0.01, cm, sd)
        bound = 10 * E_REF_NEI * np.maximum(1.0, np.abs(on_host["one"])) + np.abs(dm).max(axis=0) * 1e-8 + np.abs(ds).max(axis=0) * 1e-8 / (2 * sd)
        e = {k: float(R.err(on_dev[k], on_host[k]).max()) for k in ("fplus", "cmean", "cvar")}
        d = np.abs(on_dev["one"] - on_host["one"])
        print(f"n = {n}: host against device: {e}; lognei max {d.max():.3e}, worst share of twice the bound {np.max(d / (2 * bound)):.3e}")
        assert np.all(np.isfinite(bound)) and np.all(np.isfinite(on_dev["one"])) and np.all(np.isfinite(on_host["one"]))
        assert max(e.values()) <= 2e-8
        assert np.all(d <= 2 * bound)
