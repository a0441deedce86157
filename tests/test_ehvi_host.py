"""The two-objective expected hypervolume improvement (include/gpe_ehvi.h) — what can be held WITHOUT a device:

* the C-ABI: a header of its own, exported by libgpengine.so, bound by limbo_amd._capi;
* the accuracy of the REFERENCE every other comparison leans on: tests/ehvi_ref.py's numpy strip sum (value and four partials)
  against the same quantities in 50-digit arithmetic on the golden cases and on tail cases down to 1e-280.  f(z) = phi + z Phi loses
  about z^2 ulps to cancellation at large negative z, so the error is MEASURED: its worst is E_REF_EHVI below, and the bars of the
  device tests (tests/test_gpu_ehvi.py) are multiples of it;
* that the definition is the reference implementation's: tests/golden/ehvi2d_reference.json holds its ehvi2d's outputs beside the
  50-digit values; they agree within that implementation's own error on the file, recorded below;
* Monte Carlo, and the properties the construction promises;
* gpe_ehvi2_front (host only) against a quadratic-time front in plain python, and the front check of gpe_ehvi2_values;
* the host path of the C++ drop-in (acqui/ehvi.hpp below Params::gpu::min_n_for_gpu): tests/cpp/test_ehvi_dropin, compiled here with
  the flags of tests/cpp/Makefile, against the reference on the beliefs the driver itself reports."""
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from limbo_amd import _capi
from tests import ehvi_cases as C
from tests import ehvi_ref as R

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("gpe_ehvi2_front", "gpe_ehvi2_values", "gpe_ehvi2_batch", "gpe_ehvi_phase_ms")
# worst relative error of ref_ehvi (value and each partial, wherever the 50-digit number is >= 1e-280) against 50-digit arithmetic over
# the golden and the tail cases, measured 2026-10-20: 1.3941e-10, the value at 35 standard deviations left of the reference point (a
# result of 2.8e-275); on the golden cases alone the worst is 5.3e-12 (a value of 7e-47), and 4e-14 where the value is >= 1e-6
E_REF_EHVI = 1.40e-10
BAR = 16 * E_REF_EHVI  # the device's bar: the KG tests' factor, for the device's own erfc / exp and another summation order
# The reference implementation's ehvi2d against the 50-digit column of the golden file, measured on that file 2026-10-20.  Its cells
# subtract Sminus gausscdf1 gausscdf2 from psi1 psi2 and keep a cell only when the difference is positive, so its error is ABSOLUTE:
# at most 6.6e-12 over all 40 cases.  Relative to the value it is 4.4e-10 where the value is >= 1e-6, 4e-8 at 5e-11, and it returns 0
# for the three cases at 6e-21, 7e-47 and 4e-211 (which the rule "value >= 1e-6 psi1(r1) psi2(r2)" admits: there psi1 psi2 is tiny too).
E_GOLDEN_ABS = 7e-12
E_GOLDEN_REL = 4.5e-10  # where the value is >= 1e-6


def rel_err(got, ref):
    """max relative difference where the reference is a normal number; elsewhere `got` must be as small"""
    got, ref = np.asarray(got, dtype=float).ravel(), np.asarray(ref, dtype=float).ravel()
    big = ref >= 1e-280
    assert np.all(got >= 0) and np.all(got[~big] <= 1e-279)
    return float(np.max(np.abs(got[big] - ref[big]) / ref[big])) if big.any() else 0.0


def golden(c):
    return np.array(c["front"], dtype=float).reshape(-1, 2), c["mu"][0], c["s"][0], c["mu"][1], c["s"][1]


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_abi_lives_in_its_own_header(engine_lib):
    hs = (ROOT / "include" / "gpe_ehvi.h").read_text()
    h = (ROOT / "include" / "gpe.h").read_text()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hs), n + " is not declared in include/gpe_ehvi.h"
        assert not re.search(r"\b" + n + r"\s*\(", h), n + " must not be declared in include/gpe.h"
        assert hasattr(engine_lib.cdll, n), n + " is not exported by libgpengine.so"
        assert engine_lib.fn(n[4:]).argtypes is not None, n + " is not bound by _capi"
    assert '#include "gpe.h"' in hs
    for m in ("ehvi2_values", "ehvi2_batch", "ehvi_phase_ms"):
        assert callable(getattr(_capi.Handle, m))
    assert callable(_capi.ehvi2_front)
    assert _capi.EHVI_MAX_FRONT == 2048
    assert re.search(r"#define\s+GPE_EHVI_MAX_FRONT\s+2048\b", hs)
    assert b"k_ehvi2" in _capi.ENGINE_SO.read_bytes(), "the strip kernel is in the shipped code object"


# ------------------------------------------------------------------------------------------------ the reference's own accuracy
def test_reference_against_50_digits():
    import mpmath as mp

    cases = [(c["name"],) + golden(c) for c in C.golden_cases()] + C.tail_cases()
    worst, smallest = 0.0, 1.0
    for name, F, m1, s1, m2, s2 in cases:
        v, p = R.ref_ehvi(F, C.REF, m1, s1, m2, s2)
        ev, ep = R.mp_ehvi(F, C.REF, m1, s1, m2, s2)
        errs = []
        for got, exact in zip([v[0]] + list(p[0]), [ev] + ep):
            assert got >= 0
            if exact >= mp.mpf("1e-280"):
                errs.append(float(abs(mp.mpf(float(got)) - exact) / exact))
            else:
                assert got <= 1e-279
        if ev >= mp.mpf("1e-280"):
            smallest = min(smallest, float(ev))
        print(f"{name:20s} ehvi = {mp.nstr(ev, 6):>14s}  worst relative error {max(errs) if errs else 0.0:.3e}")
        worst = max([worst] + errs)
    print(f"worst relative error {worst:.4e} (E_REF_EHVI = {E_REF_EHVI:.4e}), smallest value held {smallest:.3e}")
    assert smallest <= 1e-270, "tail cases down to 1e-280 are among the cases"
    assert worst <= E_REF_EHVI


def test_golden_file_pins_the_definition():
    """every case of the file, none skipped: the reference implementation's output against the 50-digit strip sum, and the file's
    50-digit column against mp_ehvi as it is today"""
    cases = C.golden_cases()
    assert len(cases) == 40 and sorted({c["n"] for c in cases}) == [0, 1, 2, 3, 17, 64, 65, 300]
    worst_abs = worst_rel = 0.0
    for c in cases:
        F, m1, s1, m2, s2 = golden(c)
        assert R.is_prepared(F, c["ref"]) and tuple(c["ref"]) == C.REF
        exact, _ = R.mp_ehvi(F, C.REF, m1, s1, m2, s2, partials=False)
        base, _ = R.mp_ehvi(np.zeros((0, 2)), C.REF, m1, s1, m2, s2, partials=False)
        assert float(exact) == c["exact"] and exact >= 1e-6 * base, c["name"]
        a = abs(c["reference"] - c["exact"])
        worst_abs = max(worst_abs, a)
        assert a <= E_GOLDEN_ABS, c["name"]
        if c["exact"] >= 1e-6:
            worst_rel = max(worst_rel, a / c["exact"])
            assert a <= E_GOLDEN_REL * c["exact"], c["name"]
    print(f"reference implementation against 50 digits: worst absolute {worst_abs:.3e}, worst relative (value >= 1e-6) {worst_rel:.3e}")


MC_CASES = [(0, 0.3, 0.4, 0.2, 0.5), (1, 0.6, 0.3, 0.7, 0.2), (3, 0.2, 0.5, 0.9, 0.3), (17, 0.7, 0.25, 0.6, 0.35)]


@pytest.mark.parametrize("n,m1,s1,m2,s2", MC_CASES)
def test_reference_against_monte_carlo(n, m1, s1, m2, s2):
    F = C.concave_front(n, np.random.default_rng(50 + n))
    v, _ = R.ref_ehvi(F, C.REF, m1, s1, m2, s2)
    mean, se = R.mc_hvi(F, C.REF, m1, s1, m2, s2, draws=2_000_000, seed=n)
    print(f"n = {n}: ehvi {v[0]:.6e}, Monte Carlo {mean:.6e} +- {se:.1e} ({(v[0] - mean) / se:+.2f} standard errors)")
    assert se > 0 and abs(v[0] - mean) <= 5 * se


def test_reference_properties():
    rng = np.random.default_rng(7)
    mu1, s1, mu2, s2 = C.random_beliefs(200, rng)
    F = C.concave_front(17, rng)
    v, p = R.ref_ehvi(F, C.REF, mu1, s1, mu2, s2)
    assert np.all(v >= 0) and np.all(p >= 0), "EHVI and its partials (sums of positive terms) are >= 0"
    # n = 0: the product of the two one-sided expected improvements
    v0, _ = R.ref_ehvi(np.zeros((0, 2)), C.REF, mu1, s1, mu2, s2)
    ei = lambda m, s, t: s * (np.exp(-0.5 * ((m - t) / s) ** 2) / R.SQRT2PI + (m - t) / s * 0.5 * R.erfc(-(m - t) / s / R.SQRT2))
    ok = v0 >= 1e-100  # (ei as written cancels at large negative z)
    assert ok.sum() >= 150 and np.max(np.abs(v0 - ei(mu1, s1, C.REF[0]) * ei(mu2, s2, C.REF[1]))[ok] / v0[ok]) <= 1e-9
    # one more front point never raises a value
    assert np.all(v <= v0 * (1 + 1e-12) + 1e-300)
    for k in (0, 8, 16):
        less, _ = R.ref_ehvi(np.delete(F, k, axis=0), C.REF, mu1, s1, mu2, s2)
        assert np.all(v <= less * (1 + 1e-12) + 1e-300)
    # s1 = s2 = 0: the plain hypervolume improvement of the point mu
    z = np.zeros(len(mu1))
    vz, _ = R.ref_ehvi(F, C.REF, mu1, z, mu2, z)
    hv = R.hypervolume2(F, C.REF)
    for m in range(len(mu1)):
        G = R.pareto_front2(np.vstack([F, [[mu1[m], mu2[m]]]]), C.REF)
        assert abs(vz[m] - (R.hypervolume2(G, C.REF) - hv)) <= 1e-14, m
    assert np.max(np.abs(vz - R.hvi_points(F, C.REF, np.stack([mu1, mu2], axis=1)))) <= 1e-15
    assert np.any(vz > 0) and np.any(vz == 0)


def test_partials_against_central_differences_of_50_digits():
    """the four partials of the reference against central differences of the VALUE as the 50-digit checker forms it — step 1e-20,
    and 100 digits for the difference itself: a partial can be 1e-40 of the value (d/d s1 far above the front), which 50 digits
    minus the step's 20 would not resolve.  The truncation error is 1e-40 f''', far below the bar."""
    import mpmath as mp

    rng = np.random.default_rng(11)
    worst, held = 0.0, 0
    for n in (0, 1, 3, 17):
        F = C.concave_front(n, rng)
        mu1, s1, mu2, s2 = C.random_beliefs(6, rng)
        _, p = R.ref_ehvi(F, C.REF, mu1, s1, mu2, s2)
        for m in range(6):
            x = [mu1[m], s1[m], mu2[m], s2[m]]
            _, mp_p = R.mp_ehvi(F, C.REF, x[0], x[1], x[2], x[3])
            with mp.workdps(100):
                h = mp.mpf("1e-20")
                for k in range(4):
                    def val(t):
                        y = [mp.mpf(float(q)) for q in x]
                        y[k] += t
                        l, hh = R._strips(F, C.REF)
                        ev = lambda mu, s, t_: s * (mp.npdf((mu - t_) / s) + (mu - t_) / s * mp.ncdf((mu - t_) / s))
                        a = [ev(y[0], y[1], mp.mpf(float(t_))) for t_ in l] + [mp.mpf(0)]
                        b = [ev(y[2], y[3], mp.mpf(float(t_))) for t_ in hh]
                        return mp.fsum((a[i] - a[i + 1]) * b[i] for i in range(len(l)))
                    cd = (val(h) - val(-h)) / (2 * h)
                    if cd < mp.mpf("1e-280"):
                        continue
                    held += 1
                    assert abs(mp_p[k] - cd) / cd <= mp.mpf("1e-18"), "mp_ehvi's partials are the value's derivatives"
                    worst = max(worst, float(abs(mp.mpf(float(p[m, k])) - cd) / cd))
    print(f"partials against central differences of the 50-digit value: {held} held, worst relative error {worst:.3e}")
    assert held >= 80 and worst <= E_REF_EHVI


# ------------------------------------------------------------------------------------------------ gpe_ehvi2_front and the front check
def front_check(engine_lib, F, ref):
    """gpe_ehvi2_values with M = 0 IS the front check and needs no handle (include/gpe_ehvi.h)"""
    F = np.ascontiguousarray(np.asarray(F, dtype=float).reshape(-1, 2))
    r = np.ascontiguousarray(np.asarray(ref, dtype=float))
    return engine_lib.fn("ehvi2_values")(None, _capi._d(F), F.shape[0], _capi._d(r), None, None, None, None, 0, None, None)


def test_front_preparation(engine_lib):
    rng = np.random.default_rng(3)
    ref = (0.1, 0.2)
    for n in (0, 1, 2, 7, 100, 5000):
        P = rng.uniform(0, 1, size=(n, 2))  # dominated points, points at or below ref, unsorted
        if n >= 7:
            P[3] = P[1]  # a duplicate
            P[4] = (ref[0], 0.9)  # on ref in f1
            P[5] = (0.95, ref[1])  # on ref in f2
            P[6] = (np.inf, 0.5)  # not finite: dropped
            P[2] = (P[0, 0], P[0, 1] - 0.01)  # equal in f1, lower in f2: dominated
        rc, F = _capi.ehvi2_front(P, ref)
        assert rc == 0
        want = R.pareto_front2(P, ref) if n <= 100 else None
        assert R.is_prepared(F, ref) and front_check(engine_lib, F, ref) == 0
        if want is not None:
            assert np.array_equal(F, want), n
        else:  # every kept point is one of P's, none of P's dominates it, and every point of P above ref is dominated or kept
            keep = {tuple(p) for p in F}
            assert keep <= {tuple(p) for p in P}
            for p in P:
                if np.all(np.isfinite(p)) and p[0] > ref[0] and p[1] > ref[1]:
                    assert tuple(p) in keep or np.any((F[:, 0] >= p[0]) & (F[:, 1] >= p[1]))
    # duplicates of one point: one is kept
    rc, F = _capi.ehvi2_front(np.tile([[0.5, 0.6]], (9, 1)), ref)
    assert rc == 0 and F.tolist() == [[0.5, 0.6]]
    # a NaN is GPE_ERR_ARG, in the points and in ref
    P = rng.uniform(0.3, 1, size=(5, 2))
    P[2, 1] = np.nan
    assert _capi.ehvi2_front(P, ref, check=False)[0] == -1
    assert _capi.ehvi2_front(P[:2], (np.nan, 0.0), check=False)[0] == -1
    # the front check itself
    G = C.concave_front(9, rng)
    assert front_check(engine_lib, G, C.REF) == 0 and front_check(engine_lib, np.zeros((0, 2)), C.REF) == 0
    assert front_check(engine_lib, G[::-1], C.REF) == -1, "descending in f1"
    assert front_check(engine_lib, G[[0, 2, 1, 3]], C.REF) == -1, "unsorted"
    assert front_check(engine_lib, np.vstack([G[:3], G[2:3]]), C.REF) == -1, "a duplicate"
    assert front_check(engine_lib, G, (G[0, 0], C.REF[1])) == -1, "a front point not above ref in f1"
    assert front_check(engine_lib, G, (C.REF[0], G[-1, 1])) == -1, "a front point not above ref in f2"
    assert front_check(engine_lib, np.vstack([G, [[np.nan, -0.15]]]), C.REF) == -1
    assert front_check(engine_lib, C.concave_front(2049, rng), C.REF) == -1, "n > GPE_EHVI_MAX_FRONT"
    assert front_check(engine_lib, C.concave_front(2048, rng), C.REF) == 0


# ------------------------------------------------------------------------------------------------ the drop-in's host path
DRIVER = ROOT / "tests" / "cpp" / "test_ehvi_dropin"
NOISES = (0.01, 0.1)  # Params::kernel::noise of the driver by noise_id
FD_STEP = 1e-4


def build_driver():
    """tests/cpp/test_ehvi_dropin with the flags of tests/cpp/Makefile (that file is not this test's to change)"""
    src = DRIVER.with_suffix(".cpp")
    deps = [src, _capi.ENGINE_SO] + list((ROOT / "include").rglob("*.h*"))
    if DRIVER.exists() and all(DRIVER.stat().st_mtime >= d.stat().st_mtime for d in deps):
        return DRIVER
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Wno-unused-variable", "-I" + str(ROOT / "include" / "limbo_amd"),
                           "-I" + str(ROOT / "oracle" / "ref_build" / "shim"), "-o", str(DRIVER), str(src), "-L" + str(ROOT / "limbo_amd"),
                           "-lgpengine", "-Wl,-rpath,$ORIGIN/../../limbo_amd", "-Wl,-rpath,/opt/rocm/lib", "-lpthread"])
    return DRIVER


def run_driver(tmp_path, kind, mean, X, Y, Fp, ref, Q, noise_id=0, observation=0, hp=None, env=None):
    exe = build_driver()
    n, D = X.shape
    f = tmp_path / "in.txt"
    with open(f, "w") as fh:
        fh.write(f"{kind} {mean} {D} {n} {len(Fp)} {len(Q)} {noise_id} {int(observation)} {0 if hp is None else len(hp)} {ref[0]!r} {ref[1]!r}\n")
        if hp is not None:
            fh.write(" ".join(repr(float(v)) for v in hp) + "\n")
        for i in range(n):
            fh.write(" ".join(repr(float(v)) for v in list(X[i]) + list(Y[i])) + "\n")
        for v in list(Fp) + list(Q):
            fh.write(" ".join(repr(float(x)) for x in v) + "\n")
    r = subprocess.run([str(exe), str(f)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        out[w[0]] = np.array([float(v) for v in w[1:]])
    return out


def dropin_problem(kind, n, M, seed):
    """two competing objectives of x in [0, 1]^D with noise; the front is taken from the observations themselves"""
    D = 3 if kind == 0 else 2
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, size=(n, D))
    f = lambda V: np.stack([np.cos(1.5 * V.sum(axis=1)) + 0.3 * V[:, 0], np.sin(1.5 * V.sum(axis=1)) - 0.3 * V[:, 0]], axis=1)
    Y = f(X) + 0.05 * rng.normal(size=(n, 2))
    ref = (float(Y[:, 0].min()) - 0.1, float(Y[:, 1].min()) - 0.1)
    return X, Y, ref, rng.uniform(-0.3, 1.3, size=(M, D))  # (beyond the data: beliefs wide enough for values that do not vanish)


def with_steps(Q, h=FD_STEP):
    """Q followed by Q + h e_d and Q - h e_d for every d: one driver run gives batch() on all of them"""
    M, D = Q.shape
    out = [Q]
    for d in range(D):
        e = np.zeros(D)
        e[d] = h
        out += [Q + e, Q - e]
    return np.vstack(out)


def sd_of(s2, noise, observation):
    return np.sqrt(s2 if observation else np.maximum(s2 - noise, 0.0))


def check_dropin(got, M, D, noise, observation, bar, what):
    """the driver's numbers against the reference ON THE BELIEFS THE DRIVER REPORTS, and its gradients against central differences
    of its own batch().  bar: relative, on the values.  The gradient: step h = 1e-4 — truncation h^2 f''' / 6 = 2e-9 f''' plus rounding
    1e-16 / h — against 1e-6 max(1, |grad|): three orders of room for f''' and still six digits of the gradient."""
    T = M * (1 + 2 * D)
    front = got["front"].reshape(-1, 2)
    ref = got["ref_used"]
    assert R.is_prepared(front, ref) and abs(got["hv"][0] - R.hypervolume2(front, ref)) <= 1e-13
    mu, s2 = got["mu"].reshape(T, 2, order="F"), got["s2"]
    sd = sd_of(s2, noise, observation)
    one, _ = R.ref_ehvi(front, ref, mu[:, 0], sd, mu[:, 1], sd)
    e1 = rel_err(got["one"], one)
    two, part = R.ref_ehvi(front, ref, got["mu1"], sd_of(got["s2_1"], noise, observation), got["mu2"], sd_of(got["s2_2"], noise, observation))
    e2 = rel_err(got["two"], two)
    print(f"{what}: ehvi in [{one.min():.3e}, {one.max():.3e}], median {np.median(one):.3e}; relative error: one model {e1:.3e}, two {e2:.3e}")
    assert e1 <= bar and e2 <= bar
    assert int(got["best_one"][0]) == int(np.argmax(got["one"])) and int(got["best_two"][0]) == int(np.argmax(got["two"]))
    assert int(got["best_none"][0]) == -1
    assert np.array_equal(got["obj"], got["two"]), "the objective's batch() is batch()"
    assert rel_err(got["val"], got["two"]) <= bar, "batch_grad's values are batch()'s (beliefs from query_grad_batch, not query_batch)"
    g = got["grad"].reshape(T, D)[:M]
    val = got["val"]
    cd = np.stack([(val[M * (1 + 2 * d):M * (2 + 2 * d)] - val[M * (2 + 2 * d):M * (3 + 2 * d)]) / (2 * FD_STEP) for d in range(D)], axis=1)
    dg = float(np.max(np.abs(g - cd)))
    print(f"{what}: max|grad| {np.max(np.abs(g)):.3e}, max|grad - central difference| {dg:.3e}")
    assert np.max(np.abs(g)) > 1e-4, "a gradient that is zero everywhere shows nothing"
    assert dg <= 1e-6 * max(1.0, float(np.max(np.abs(g))))
    assert abs(got["single"][0] - val[0]) <= bar * val[0] and np.max(np.abs(got["single"][1:] - g[0])) <= 1e-6 * max(1.0, float(np.max(np.abs(g))))
    return one, two, part


# (kind, mean, n, noise_id, observation): SE-ARD with the Data mean, latent; Matern-5/2, the observation's variance; a constant mean
HOST_CASES = [(0, 0, 60, 0, 0), (1, 0, 40, 1, 1), (0, 2, 200, 0, 0)]


@pytest.mark.parametrize("kind,mean,n,noise_id,observation", HOST_CASES)
def test_dropin_host_path(tmp_path, kind, mean, n, noise_id, observation):
    M = 12
    X, Y, ref, Q = dropin_problem(kind, n, M, 100 * kind + 10 * mean + n)
    got = run_driver(tmp_path, kind, mean, X, Y, Y, ref, with_steps(Q), noise_id, observation,
                     env={"LIMBO_AMD_MIN_N_FOR_GPU": str(1 << 20), "LIMBO_AMD_HOST_BATCH_CROSSOVER": str(1 << 40)})
    assert np.all(got["host_resident"] == 1)
    got["ref_used"] = ref
    assert np.array_equal(got["front"].reshape(-1, 2), R.pareto_front2(Y, ref))
    one, _, _ = check_dropin(got, M, Q.shape[1], NOISES[noise_id], observation, 10 * E_REF_EHVI, f"host n = {n}")
    assert np.mean(one >= 1e-6) >= 0.25, "values that all vanish show little"


def test_dropin_prior(tmp_path):
    """no samples: the prior's beliefs (mean functor, k(v, v)), an empty front: the product of two expected improvements"""
    Q = np.random.default_rng(5).uniform(0, 1, size=(6, 3))
    got = run_driver(tmp_path, 0, 2, np.zeros((0, 3)), np.zeros((0, 2)), np.zeros((0, 2)), (0.5, 0.2), with_steps(Q))
    assert got["front"].size == 0 and got["hv"][0] == 0.0
    mu, s2 = got["mu"].reshape(-1, 2, order="F"), got["s2"]
    sd = sd_of(s2, NOISES[0], 0)
    want, _ = R.ref_ehvi(np.zeros((0, 2)), (0.5, 0.2), mu[:, 0], sd, mu[:, 1], sd)
    assert rel_err(got["one"], want) <= 10 * E_REF_EHVI and rel_err(got["two"], want) <= 10 * E_REF_EHVI
    assert np.all(got["one"] > 0)
