"""Max-value entropy search in the log domain (include/gpe_mes.h) — what can be held WITHOUT a device:

* the C-ABI: a header of its own, exported by libgpengine.so, bound by limbo_amd._capi, the kernel in the shipped code object;
* the argument statuses that need no device;
* the accuracy of the REFERENCE every other comparison leans on: tests/mes_ref.py's numpy / scipy ref_mes (value, terms, partials)
  against the same quantities in 60-digit arithmetic.  The error is MEASURED: its worst is E_REF_MES below, and the bar of the device
  tests (tests/test_gpu_mes.py) is a multiple of it.  The measure is |got - truth| / max(1, |truth|) throughout;
* the partials as central differences of the reference value;
* the plateau: the per-sample term as written is NaN at g = -39 and 0 at g = +39 where ref_mes is finite with non-zero partials;
* the host path of the C++ drop-in (acqui/mes.hpp below Params::gpu::min_n_for_gpu): tests/cpp/test_mes_dropin, compiled here with
  the flags of tests/cpp/Makefile, against the reference on the beliefs the driver itself reports."""
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from limbo_amd import _capi
from tests import mes_ref as R

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("gpe_mes_values", "gpe_mes_batch", "gpe_mes_phase_ms")
# worst error of ref_mes (value, every term, every partial; |got - truth| / max(1, |truth|)) against 60-digit arithmetic over the
# cases of test_reference_against_60_digits, measured 2026-10-20: 1.3637e-13, the partial d/d mu at g = -2.999, s = 0.05, K = J = 1
# — just inside the crossover, the last stretch of the direct form, where 1 + g (g + lambda) = 1 - x (lambda - x) cancels 11 times,
# log Phi carries scipy's few ulps and 1 / s = 20 scales the partial; outside the crossover the worst is 1e-14.
E_REF_MES = 1.37e-13
# The device's bar: the KG, EHVI and CEI tests' factor, for the device's own exp, erfc and log: 2.2e-12.  Why the kernel's worst spot
# stays under it.  (a) Inside the crossover the same cancellation: 11 x (the few ulps of the device's exp, erfc and log + 3
# roundings, say 10) x 1.1e-16 = 1.2e-14 of r, times 1 / s.  The measure divides by max(1, |ref|) and the partial is r / s itself, so
# the error stays 1.2e-14 relative whenever |r / s| >= 1, and below that it is smaller absolutely.  (b) On the tails every piece is a
# positive sum, a quotient or one log; what grows is the weight exp(log t - max): log t reaches -800 at g = 40 and carries 0.5 ulp of
# itself, 800 x 1.1e-16 = 9e-14 relative in a weight — but the weights of one output share that rounding to first order when their g
# lie close, and over g spread by 3 (the tests' beliefs) the worst pair differs by 40 x 3 x 1.1e-16 = 1.3e-14.  (c) The sums run in
# another order than numpy's: K x 1.1e-16 x the spread of positive terms, 1e-13 at K = 1024 before the tree, 1e-15 after it (a tree
# of depth 10 + 16 serial terms).  Together a few 1e-14, forty times below BAR.
BAR = 16 * E_REF_MES
FD_STEP = 1e-4  # the EHVI tests' step


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_abi_lives_in_its_own_header(engine_lib):
    hs = (ROOT / "include" / "gpe_mes.h").read_text()
    h = (ROOT / "include" / "gpe.h").read_text()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hs), n + " is not declared in include/gpe_mes.h"
        assert not re.search(r"\b" + n + r"\s*\(", h), n + " must not be declared in include/gpe.h"
        assert hasattr(engine_lib.cdll, n), n + " is not exported by libgpengine.so"
        assert engine_lib.fn(n[4:]).argtypes is not None, n + " is not bound by _capi"
    assert '#include "gpe.h"' in hs
    for m in ("mes_values", "mes_batch", "mes_phase_ms"):
        assert callable(getattr(_capi.Handle, m))
    assert _capi.MES_MAX_OUTPUTS == R.MAX_OUTPUTS == 8 and _capi.MES_MAX_SAMPLES == R.MAX_SAMPLES == 1024
    assert re.search(r"#define\s+GPE_MES_MAX_OUTPUTS\s+8\b", hs) and re.search(r"#define\s+GPE_MES_MAX_SAMPLES\s+1024\b", hs)
    assert b"k_mes" in _capi.ENGINE_SO.read_bytes(), "the kernel is in the shipped code object"
    csrc = ROOT / "limbo_amd" / "csrc"
    src = (csrc / "mes.hip").read_text()
    # the crossover is logh.h's, the one the kernel uses: it includes the header, branches on LOGH_XC and defines none of its own
    assert '#include "logh.h"' in src and "LOGH_XC" in src and not re.search(r"_XC\s*=", src)
    assert re.search(r"LOGH_XC\s*=\s*3\.0\b", (csrc / "logh.h").read_text()) and R.CROSSOVER == 3.0, "the tests probe the kernel's crossover"
    # ... and on the host normal.hpp's: the host form includes it and defines neither a crossover nor a depth of its own
    gp = ROOT / "include" / "limbo_amd" / "limbo" / "model" / "gp"
    normal, host = (gp / "normal.hpp").read_text(), (gp / "mes.hpp").read_text()
    assert re.search(r"\bcrossover\s*=\s*3\.0\b", normal) and re.search(r"\bdepth\s*=\s*60\b", normal) and R.CROSSOVER == 3.0
    assert "#include <limbo/model/gp/normal.hpp>" in host and not re.search(r"\b(crossover|depth)\s*=", host)


def test_argument_statuses_without_a_device(engine_lib):
    """the checks precede everything that needs the device: with M = 0 the call IS the check and takes no handle"""
    f = engine_lib.fn("mes_values")
    d = _capi._d

    def check(J=1, K=4, ystar="ok", M=0):
        y = np.linspace(-1.0, 1.0, max(J * K, 1)) if isinstance(ystar, str) else np.ascontiguousarray(np.asarray(ystar, dtype=float))
        return f(None, J, K, d(y), None, None, M, None, None, None)

    assert check() == 0 and check(J=8, K=1024) == 0 and check(J=8, K=1) == 0
    for J in (0, -1, 9):
        assert check(J=J) == -1, f"J = {J}"
    for K in (0, -1, 1025):
        assert check(K=K) == -1, f"K = {K}"
    for bad in (np.inf, -np.inf, np.nan):
        assert check(J=2, K=2, ystar=[0.1, 0.2, bad, 0.3]) == -1, "a ystar that is not finite"
    assert f(None, 1, 4, None, None, None, 0, None, None, None) == -1, "ystar missing"
    assert check(M=-1) == -1
    assert check(M=3) == -1, "NULL where data is needed"
    g = engine_lib.fn("mes_batch")
    assert g(None, 1, None, 1, None, None, 0, None, 0.0, None, None, None, None, None) == -1, "no handle"
    assert engine_lib.fn("mes_phase_ms")(None, None) == -1


# ------------------------------------------------------------------------------------------------ the reference's own accuracy
def grid_points():
    """g: a grid over [-40, 40], the points +-1e2 .. +-1e8, both sides of +-x_c at 1e-9 and 1e-3"""
    x = R.CROSSOVER
    edge = [sg * (x + d) for sg in (-1.0, 1.0) for d in (-1e-3, -1e-9, 0.0, 1e-9, 1e-3)]
    return np.concatenate([np.linspace(-40.0, 40.0, 161), 10.0 ** np.arange(2, 9), -(10.0 ** np.arange(2, 9)), edge])


def test_reference_against_60_digits():
    P = grid_points()
    S = (0.05, 1.0, 11.0)
    worst, where = 0.0, None

    def one(ystar, mu, s, tag):
        nonlocal worst, where
        v, t, p = R.ref_mes(ystar, [mu], [s])
        ev, et, ep = R.mp_mes(ystar, mu, s, dps=60)
        got = np.concatenate([v, t[0], p[0]])
        exact = np.array([float(a) for a in [ev] + et + ep])
        assert np.all(np.isfinite(got)), tag
        e = R.err(got, exact)
        if e.max() > worst:
            worst, where = float(e.max()), tag + (int(np.argmax(e)),)

    # K = J = 1: every grid point alone, at every s
    for g in P:
        for s in S:
            one(np.array([[0.3 + g * s]]), [0.3], [s], (1, 1, float(g), s))
    # K in {3, 64}, J in {1, 2, 8}: the samples of an output spread by up to 3 about a grid point (what sampled maxima of one
    # output do); the outputs' centres walk through the grid
    rng = np.random.default_rng(7)
    for K in (3, 64):
        for J in (1, 2, 8):
            for i in range(0, len(P), 1 if K == 3 else 12):
                mu = rng.uniform(-1, 1, J)
                s = np.array([S[(i + j) % 3] for j in range(J)])
                c = np.array([P[(i + 11 * j) % len(P)] for j in range(J)])
                g = c[None, :] + np.where(np.abs(c) > 50, 0.0, 1.0)[None, :] * rng.uniform(-1.5, 1.5, (K, J))
                one(mu[None, :] + g * s[None, :], mu, s, (K, J, float(c[0]), float(s[0])))
    print(f"worst error {worst:.4e} at (K, J, g, s, slot) = {where} (E_REF_MES = {E_REF_MES:.4e})")
    assert worst <= E_REF_MES


def test_asymptotes_at_1e100():
    """|g| = 1e100: finite, and the limits: g -> -inf: t -> log x + log sqrt(2 pi) - 1/2, t' -> -1 / x; g -> +inf: log t -> -g^2 / 2
    - log sqrt(2 pi) + log(g / 2 + 1 / g), t' / t -> -g"""
    x = 1e100
    for s in (0.05, 1.0, 11.0):
        v, t, p = R.ref_mes([[-x * s]], [[0.0]], [[s]])
        tv = np.log(x) + R.LOG_SQRT2PI - 0.5
        assert np.all(np.isfinite(np.concatenate([v, t[0], p[0]])))
        assert abs(v[0] - np.log(tv)) <= 4e-16 * abs(np.log(tv)) and t[0, 0] == v[0]
        assert abs(p[0, 0] - (1.0 / x) / tv / s) <= 1e-15 * p[0, 0] and abs(p[0, 1] + 1.0 / tv / s) <= 1e-15 * abs(p[0, 1])
        v, t, p = R.ref_mes([[x * s]], [[0.0]], [[s]])
        assert np.all(np.isfinite(np.concatenate([v, t[0], p[0]])))
        assert abs(v[0] + 0.5 * x * x) <= 1e-15 * 0.5 * x * x
        assert abs(p[0, 0] - x / s) <= 1e-15 * x / s and abs(p[0, 1] - x * x / s) <= 1e-15 * x * x / s
    lt, r = R.log_t(np.array([-x, x]))
    assert np.all(np.isfinite(lt)) and abs(r[0] * (np.log(x) + R.LOG_SQRT2PI - 0.5) + 1.0 / x) <= 1e-115 and abs(r[1] + x) <= 1e-15 * x


def test_partials_are_central_differences():
    """the reference's partials against central differences of its own value at the EHVI tests' step h = 1e-4: truncation h^2 f''' / 6
    with f''' up to a few hundred at s = 0.3 (1 / s^3) plus rounding 1e-16 |f| / h: within 1e-5 max(1, |partial|)"""
    rng = np.random.default_rng(3)
    for K, J in ((1, 1), (10, 1), (64, 3), (7, 8)):
        M = 40
        c = rng.uniform(-12, 12, (M, J))
        s = rng.uniform(0.3, 2.0, (M, J))
        mu = rng.uniform(-1, 1, (M, J))
        ystar = rng.uniform(-1.0, 1.0, (K, J))
        mu = ystar.mean(axis=0)[None, :] - c * s  # g about c
        v, t, p = R.ref_mes(ystar, mu, s)
        assert np.all(np.isfinite(p)) and np.all(p[:, :J] >= 0), "d/d mu >= 0"
        for col in range(2 * J):
            up_mu, dn_mu, up_s, dn_s = mu.copy(), mu.copy(), s.copy(), s.copy()
            (up_mu if col < J else up_s)[:, col % J] += FD_STEP
            (dn_mu if col < J else dn_s)[:, col % J] -= FD_STEP
            cd = (R.ref_mes(ystar, up_mu, up_s)[0] - R.ref_mes(ystar, dn_mu, dn_s)[0]) / (2 * FD_STEP)
            assert np.max(np.abs(cd - p[:, col]) / np.maximum(1.0, np.abs(cd))) <= 1e-5, (K, J, col)


def test_plateau_is_shown():
    """the per-sample term as written: NaN (0 / 0) at g = -39, exactly 0 — flat — at g = +39; the reference there: finite, with
    non-zero partials"""
    with np.errstate(all="ignore"):
        tb = R.textbook_t(np.array([-39.0, 39.0]))
    assert np.isnan(tb[0]) and tb[1] == 0.0
    for g in (-39.0, 39.0):
        v, t, p = R.ref_mes([[g]], [[0.0]], [[1.0]])
        assert np.isfinite(v[0]) and np.all(np.isfinite(p)) and np.all(p != 0.0), g
    v, _, _ = R.ref_mes([[39.0]], [[0.0]], [[1.0]])
    assert v[0] < -745.0, "finite where exp() of it has underflowed"
    e = R.mp_mes(np.array([[39.0]]), [0.0], [1.0])[0]
    assert abs(v[0] - float(e)) <= E_REF_MES * abs(float(e))


# ------------------------------------------------------------------------------------------------ the drop-in's host path
DRIVER = ROOT / "tests" / "cpp" / "test_mes_dropin"
NOISES = (0.01, 0.1)  # Params::kernel::noise of the driver by noise_id
HOST_ENV = {"LIMBO_AMD_MIN_N_FOR_GPU": str(1 << 20), "LIMBO_AMD_HOST_BATCH_CROSSOVER": str(1 << 40)}  # test_cei_host.py's


def build_driver():
    """tests/cpp/test_mes_dropin with the flags of tests/cpp/Makefile (that file is not this test's to change)"""
    src = DRIVER.with_suffix(".cpp")
    deps = [src, _capi.ENGINE_SO] + list((ROOT / "include").rglob("*.h*"))
    if DRIVER.exists() and all(DRIVER.stat().st_mtime >= d.stat().st_mtime for d in deps):
        return DRIVER
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Wno-unused-variable", "-I" + str(ROOT / "include" / "limbo_amd"),
                           "-I" + str(ROOT / "oracle" / "ref_build" / "shim"), "-o", str(DRIVER), str(src), "-L" + str(ROOT / "limbo_amd"),
                           "-lgpengine", "-Wl,-rpath,$ORIGIN/../../limbo_amd", "-Wl,-rpath,/opt/rocm/lib", "-lpthread"])
    return DRIVER


def run_driver(tmp_path, kind, mean, X, Y, Q, K, seed, noise_id=0, observation=0, hp=None, search=0, env=None):
    exe = build_driver()
    n, D = X.shape
    f = tmp_path / "in.txt"
    with open(f, "w") as fh:
        fh.write(f"{kind} {mean} {D} {n} {Y.shape[1]} {len(Q)} {noise_id} {int(observation)} {0 if hp is None else len(hp)} {K} {seed} {int(search)}\n")
        if hp is not None:
            fh.write(" ".join(repr(float(v)) for v in hp) + "\n")
        for i in range(n):
            fh.write(" ".join(repr(float(v)) for v in list(X[i]) + list(Y[i])) + "\n")
        for v in Q:
            fh.write(" ".join(repr(float(x)) for x in v) + "\n")
    r = subprocess.run([str(exe), str(f)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return {ln.split()[0]: np.array([float(v) for v in ln.split()[1:]]) for ln in r.stdout.splitlines()}


def dropin_problem(D, n, P, M, seed, amplitude=3.0):
    """P smooth objectives of x in [0, 1]^D with noise; candidates in and a little around the box"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, size=(n, D))
    W = rng.uniform(0.5, 1.5, size=(P, D))
    Y = np.column_stack([amplitude * np.cos(1.5 * X @ W[p] + p) for p in range(P)]) + 0.05 * rng.normal(size=(n, P))
    return X, Y, rng.uniform(-0.1, 1.1, size=(M, D))


def with_steps(Q, h=FD_STEP):
    """Q followed by Q + h e_d and Q - h e_d for every d: one driver run gives batch() on all of them"""
    out = [Q]
    for d in range(Q.shape[1]):
        e = np.zeros(Q.shape[1])
        e[d] = h
        out += [Q + e, Q - e]
    return np.vstack(out)


def check_dropin(got, M, D, P, K, noise, observation, what):
    """the driver's numbers against the reference ON THE BELIEFS THE DRIVER REPORTS, its gradients against central differences of
    its own batch() (step 1e-4: truncation 2e-9 f''' plus rounding 1e-16 |f| / h, against 1e-6 max(1, |grad|), test_cei_host.py's
    bound), and the samples of the maximum: reproducible for a seed, PathSet::argmax's fmax on the same draws"""
    T = M * (1 + 2 * D)
    ystar = got["ystar"].reshape(K, P, order="F")
    assert np.array_equal(got["ystar"], got["ystar_again"]) and np.array_equal(got["ystar"], got["drawn"]), "reproducible for a seed"
    assert not np.array_equal(got["ystar"], got["ystar_other"]), "another seed, other draws"
    assert np.array_equal(got["ystar"], got["ystar_direct"]), "max_value_samples is PathSet::argmax's fmax on the same draws"
    assert np.all(np.isfinite(ystar)) and np.all(got["ystar"] >= got["path_at_samples"]), "the maximum over more points is no smaller"
    mu = got["mu"].reshape(T, P, order="F")
    sd = np.sqrt(got["s2"] if observation else np.maximum(got["s2"] - noise, 0.0))
    v, t, p = R.ref_mes(ystar, mu, np.tile(sd[:, None], (1, P)))
    e1 = max(R.err(got["one"], v).max(), R.err(got["terms_one"].reshape(T, P, order="F"), t).max(),
             R.err(got["part_one"].reshape(T, 2 * P, order="F"), p).max())
    print(f"{what}: logmes in [{v.min():.3e}, {v.max():.3e}], median {np.median(v):.3e}; error {e1:.3e}")
    assert e1 <= BAR and np.all(np.isfinite(v))
    assert np.array_equal(got["one"], got["one_again"]) and np.array_equal(got["obj"], got["one"]), "mes_batch and the objective's batch()"
    assert int(got["best_one"][0]) == int(np.argmax(got["one"])) and int(got["best_none"][0]) == -1
    v1, _, _ = R.ref_mes(ystar[:, :1], mu[:, :1], sd[:, None])
    assert R.err(got["first"], v1).max() <= BAR, "output 0 alone through outs"
    val = got["val"]
    assert R.err(val, v).max() <= BAR, "batch_grad's values are batch()'s (beliefs from query_grad_batch, not query_batch)"
    g = got["grad"].reshape(T, D)[:M]
    one = got["one"]
    cd = np.stack([(one[M * (1 + 2 * d):M * (2 + 2 * d)] - one[M * (2 + 2 * d):M * (3 + 2 * d)]) / (2 * FD_STEP) for d in range(D)], axis=1)
    dg = float(np.max(np.abs(g - cd)))
    print(f"{what}: max|grad| {np.max(np.abs(g)):.3e}, max|grad - central difference| {dg:.3e}")
    assert np.max(np.abs(g)) > 1e-4, "a gradient that is zero everywhere shows nothing"
    assert dg <= 1e-6 * max(1.0, float(np.max(np.abs(g))))
    assert R.err(got["single"][0], val[0]) <= BAR and np.max(np.abs(got["single"][1:] - g[0])) <= 1e-6 * max(1.0, float(np.max(np.abs(g))))
    # the plain value: exp(logmes), its gradient exp(logmes) times the logarithm's
    assert np.all(np.abs(got["plain"] - np.exp(one)) <= 4 * np.finfo(float).eps * np.exp(one))
    assert np.all(np.abs(got["plain_val"] - np.exp(val)) <= 4 * np.finfo(float).eps * np.exp(val))
    pg = got["plain_grad"].reshape(T, D)
    assert np.all(np.abs(pg - got["plain_val"][:, None] * got["grad"].reshape(T, D)) <= 1e-14 * np.abs(pg) + 1e-300)
    return v


# (kind, P, K, noise_id, observation): SE-ARD with the Data mean, one and three objectives; Matern-5/2, the observation's variance
HOST_CASES = [(0, 1, 8, 0, 0), (0, 3, 16, 0, 0), (1, 2, 5, 1, 1)]


@pytest.mark.parametrize("kind,P,K,noise_id,observation", HOST_CASES)
def test_dropin_host_path(tmp_path, kind, P, K, noise_id, observation):
    M, D, n = 12, 3, 40
    X, Y, Q = dropin_problem(D, n, P, M, 100 * kind + 10 * P + noise_id)
    got = run_driver(tmp_path, kind, 0, X, Y, with_steps(Q), K, 11, noise_id, observation, env=HOST_ENV)
    assert np.all(got["host_resident"] == 1)
    check_dropin(got, M, D, P, K, NOISES[noise_id], observation, f"host P = {P}")
