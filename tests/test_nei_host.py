"""Noisy expected improvement in the log domain, everything that needs no GPU (include/gpe_nei.h).

* the ABI lives in a header of its own, is exported and bound; the argument checks precede everything that needs the device;
* tests/nei_ref.py's ref_lognei — the numpy / scipy reference every device test compares against — is itself compared against the
  same quantity in 50-digit arithmetic.  The error is MEASURED: its worst is E_REF_NEI below, and the device's bar is derived from it;
* ref_pipeline's conditional beliefs are the posterior of the augmented model of order N + B (mpmath), once, at N = 40, B = 9;
* the special rows: sd = 0, -inf, +inf, NaN."""
import re
from pathlib import Path

import numpy as np

from limbo_amd import _capi
from oracle import np_oracle as O
from tests import nei_ref as R

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("gpe_lognei_values", "gpe_lognei_batch", "gpe_nei_phase_ms")
# worst error of ref_lognei (value and every term; |got - truth| / max(1, |truth|)) against 50-digit arithmetic over the cases of
# test_reference_against_50_digits, measured 2026-10-20: 3.1412e-15, a term of the S = 65 case around
# z = -2.999 with sd = 10 (slot 44) — beside the crossover, on the direct form's side, where h = phi - |z| Q cancels 11.6 times; the
# partials that make E_REF_CEI eight times larger are not part of this value
E_REF_NEI = 3.15e-15
# The device's bar, the project's factor for a kernel given equal inputs (tests/test_cei_host.py: the same forms of log h, the same
# cancellation at the crossover; the log-mean-exp adds S positive numbers <= 1, the largest equal to 1)
BAR = 16 * E_REF_NEI


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_abi_lives_in_its_own_header(engine_lib):
    hs = (ROOT / "include" / "gpe_nei.h").read_text()
    h = (ROOT / "include" / "gpe.h").read_text()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hs), n + " is not declared in include/gpe_nei.h"
        assert not re.search(r"\b" + n + r"\s*\(", h), n + " must not be declared in include/gpe.h"
        assert hasattr(engine_lib.cdll, n), n + " is not exported by libgpengine.so"
        assert engine_lib.fn(n[4:]).argtypes is not None, n + " is not bound by _capi"
    assert '#include "gpe.h"' in hs
    for m in ("lognei_values", "lognei_batch", "nei_phase_ms"):
        assert callable(getattr(_capi.Handle, m))
    assert _capi.NEI_MAX_BASELINE == R.MAX_BASELINE == 1024 and _capi.NEI_MAX_SAMPLES == R.MAX_SAMPLES == 1024
    assert re.search(r"#define\s+GPE_NEI_MAX_BASELINE\s+1024\b", hs) and re.search(r"#define\s+GPE_NEI_MAX_SAMPLES\s+1024\b", hs)
    blob = _capi.ENGINE_SO.read_bytes()
    assert b"k_lognei" in blob and b"k_nei_cond" in blob and b"k_nei_colmax" in blob, "the kernels are in the shipped code object"
    # log h is shared with cei.hip through one header, not copied
    csrc = ROOT / "limbo_amd" / "csrc"
    for f in ("cei.hip", "nei.hip"):
        src = (csrc / f).read_text()
        assert '#include "logh.h"' in src and "cei_log_h(" in src and not re.search(r"void\s+cei_log_h\s*\(", src), f
    assert re.search(r"LOGH_XC\s*=\s*3\.0\b", (csrc / "logh.h").read_text()), "the tests probe the kernel's crossover (tests/cei_ref.py: CROSSOVER)"


def test_argument_statuses_without_a_device(engine_lib):
    """the checks precede everything that needs the device: with M = 0 the call IS the check and takes no handle"""
    f = engine_lib.fn("lognei_values")
    d = _capi._d

    def check(fplus=(0.5,), xi=0.0, M=0, S=None, ldm=None):
        t = np.ascontiguousarray(np.asarray(fplus, dtype=float))
        S = len(t) if S is None else S
        return f(None, S, d(t) if len(t) else None, xi, None, S if ldm is None else ldm, None, M, None, None)

    assert check() == 0 and check(fplus=np.zeros(1024)) == 0
    assert check(fplus=np.zeros(1025)) == -1, "S = 1025"
    assert check(fplus=(), S=0) == -1 and check(fplus=(), S=2) == -1, "S = 0; fplus missing"
    for bad in (np.inf, -np.inf, np.nan):
        assert check(fplus=(0.1, bad)) == -1, "an fplus that is not finite"
        assert check(xi=bad) == -1, "an xi that is not finite"
    assert check(fplus=(0.1, 0.2), ldm=1) == -1, "ldm < S"
    assert check(M=-1) == -1
    assert check(M=3) == -1, "NULL where data is needed"
    g = engine_lib.fn("lognei_batch")
    assert g(None, 0, None, 1, None, 0.0, None, 1, 0.0, None, 0, None, None, None, None, None, None, None, 1) == -1, "no handle"
    assert engine_lib.fn("nei_phase_ms")(None, None) == -1


# ------------------------------------------------------------------------------------------------ the reference's own accuracy
Z_LEVELS = [-1e100, -1e8, -1e4, -300.0, -38.6, -30.0, -10.0, -3.001, -3.0, -2.999, -1.0, 0.0, 1.0, 3.0, 10.0, 40.0]
SDS = [1e-3, 0.05, 1.0, 10.0]


def grid_case(S, z0, sd, seed):
    """S samples whose z lie around z0 (within 2, or within 2e-3 |z0| beyond |z0| = 100): fplus in [0.3, 0.5], xi = 0.01"""
    rng = np.random.default_rng(seed)
    fplus = rng.uniform(0.3, 0.5, S)
    z = z0 + rng.uniform(-2.0, 2.0, S) * (1.0 if abs(z0) <= 100 else 1e-3 * abs(z0))
    z[0] = z0
    return fplus, 0.01, (fplus + 0.01 + z * sd)[:, None], np.array([sd])


def mixed_case(S, sd, seed):
    """z spread over [-30, 6]: the terms of one candidate differ by hundreds"""
    rng = np.random.default_rng(seed)
    fplus = rng.uniform(0.3, 0.5, S)
    z = rng.uniform(-30.0, 6.0, S)
    return fplus, 0.01, (fplus + 0.01 + z * sd)[:, None], np.array([sd])


def test_reference_against_50_digits():
    worst, where = 0.0, None
    cases = []
    for S in (1, 2, 64, 65):
        levels = Z_LEVELS if S <= 2 else Z_LEVELS[::3] + [-3.0]
        for i, z0 in enumerate(levels):
            for j, sd in enumerate(SDS if S <= 2 else (SDS[i % 4],)):
                cases.append((S, z0, sd, grid_case(S, z0, sd, 1000 * S + 10 * i + j)))
        for j, sd in enumerate(SDS[:2] if S > 2 else SDS):
            cases.append((S, "mixed", sd, mixed_case(S, sd, 77 * S + j)))
    for S, z0, sd, (fplus, xi, cm, csd) in cases:
        v, t = R.ref_lognei(fplus, xi, cm, csd)
        ev, et = R.mp_lognei(fplus, xi, cm[:, 0], sd)
        got = np.concatenate([v, t[:, 0]])
        exact = np.array([float(x) for x in [ev] + et])
        assert np.all(np.isfinite(got)), (S, z0, sd)
        e = R.err(got, exact)
        if e.max() > worst:
            worst, where = float(e.max()), (S, z0, sd, int(np.argmax(e)))
    print(f"{len(cases)} cases; worst error {worst:.4e} at (S, z, sd, slot) = {where} (E_REF_NEI = {E_REF_NEI:.4e})")
    assert worst <= E_REF_NEI


def test_reference_special_rows():
    fplus, xi = np.array([0.5, 0.25, 0.0]), 0.25
    cm = np.zeros((3, 7))
    sd = np.ones(7)
    cm[:, 1], sd[1] = fplus + xi + np.array([0.5, -0.5, 2.0]), 0.0  # sd = 0: the improvement itself where there is one
    cm[:, 2], sd[2] = fplus + xi - 1.0, 0.0  # ... none anywhere: -inf
    cm[:, 3] = -np.inf
    cm[1, 4] = np.inf
    cm[2, 5] = np.nan
    sd[6] = np.nan
    v, t = R.ref_lognei(fplus, xi, cm, sd)
    assert np.isfinite(v[0]) and np.all(np.isfinite(t[:, 0]))
    assert np.allclose(t[[0, 2], 1], np.log([0.5, 2.0]), rtol=0, atol=1e-15) and t[1, 1] == -np.inf
    assert abs(v[1] - np.log((0.5 + 2.0) / 3.0)) <= 1e-15
    assert v[2] == -np.inf and v[3] == -np.inf and v[4] == np.inf
    assert np.isnan(v[5]) and np.all(np.isnan(t[:, 5])) and np.isnan(v[6])
    # 1e100 standard deviations below: finite
    v, t = R.ref_lognei(fplus, xi, (fplus + xi - 1e100)[:, None], [1.0])
    assert np.isfinite(v[0]) and v[0] < -1e199
    # S = 1: the term itself
    v, t = R.ref_lognei([0.4], 0.0, [[0.1]], [0.3])
    assert v[0] == t[0, 0]


def test_partials_are_the_terms_derivatives():
    rng = np.random.default_rng(3)
    S, M = 5, 40
    fplus = rng.uniform(0.3, 0.5, S)
    sd = 10 ** rng.uniform(-1.3, 0.7, M)
    z = rng.uniform(-12, 6, (S, M))
    cm = fplus[:, None] + z * sd[None, :]
    dm, ds = R.term_partials(fplus, 0.0, cm, sd)
    h = 1e-6
    tp, tm = R.ref_lognei(fplus, 0.0, cm + h, sd)[1], R.ref_lognei(fplus, 0.0, cm - h, sd)[1]
    assert np.max(np.abs((tp - tm) / (2 * h) - dm) / np.maximum(1.0, np.abs(dm))) <= 1e-6
    tp, tm = R.ref_lognei(fplus, 0.0, cm, sd * (1 + h))[1], R.ref_lognei(fplus, 0.0, cm, sd * (1 - h))[1]
    assert np.max(np.abs((tp - tm) / (2 * h * sd[None, :]) - ds) / np.maximum(1.0, np.abs(ds))) <= 1e-6


# ------------------------------------------------------------------------------------------------ the pipeline's conditioning
def test_pipeline_is_the_augmented_model():
    """N = 40, B = 9, S = 3, M = 6, SE-ARD, D = 3: (cmean, cvar) of ref_pipeline against the posterior of the model that also holds
    the fantasies (Xb, F[:, s]) with noise variance jitter, in 50 digits.  Bars: the conditioning of the augmented matrix (noise
    0.01: below 1e4) times LAPACK's rounding, 1e-10 — the issue's numpy experiment gave 3e-13 and 2e-15."""
    rng = np.random.default_rng(11)
    N, B, S, M, D = 40, 9, 3, 6, 3
    X = rng.random((N, D))
    y = np.sin(3.0 * X @ rng.random(D)) + 0.1 * rng.standard_normal(N)
    om = (y - y.mean())[:, None]
    th = np.concatenate([np.log(np.full(D, 0.4)), [0.0]])
    Xb = X[np.argsort(-om[:, 0])[:B]]
    Z = rng.standard_normal((B, S))
    Xc = rng.random((M, D))
    ref = R.ref_pipeline(O.SE_ARD, th, 0.01, X, om, 0, Xb, None, 1e-6, Z, 0.0, Xc, None)
    mean, var = R.mp_augmented(O.SE_ARD, th, 0.01, X, om[:, 0], Xb, ref["F"], 1e-6, Xc)
    e_m, e_v = np.max(np.abs(ref["cmean"] - mean)), np.max(np.abs(ref["cvar"] - var))
    print(f"max|cmean - augmented| {e_m:.3e}, max|cvar - augmented| {e_v:.3e}; cvar in [{var.min():.3e}, {var.max():.3e}]")
    assert e_m <= 1e-10 and e_v <= 1e-10
    assert np.all(ref["cvar"] <= ref["var"] + 1e-15), "conditioning never adds variance"
    assert np.array_equal(ref["fplus"], ref["F"].max(axis=0))


# ------------------------------------------------------------------------------------------------ the C++ drop-in
import os  # noqa: E402
import subprocess  # noqa: E402

DRIVER = ROOT / "tests" / "cpp" / "test_nei_dropin"
DROPIN_NOISE, DROPIN_JITTER, DROPIN_XI = 0.01, 1e-6, 0.01  # the driver's constants
HOST_ENV = {"LIMBO_AMD_MIN_N_FOR_GPU": "1000000", "LIMBO_AMD_HOST_BATCH_CROSSOVER": "1000000000"}  # nothing touches the device


def build_driver():
    """tests/cpp/test_nei_dropin with the flags of tests/cpp/Makefile (that file is not this test's to change)"""
    src = DRIVER.with_suffix(".cpp")
    deps = [src, _capi.ENGINE_SO] + list((ROOT / "include").rglob("*.h*"))
    if DRIVER.exists() and all(DRIVER.stat().st_mtime >= d.stat().st_mtime for d in deps):
        return DRIVER
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Wno-unused-variable", "-I" + str(ROOT / "include" / "limbo_amd"),
                           "-I" + str(ROOT / "oracle" / "ref_build" / "shim"), "-o", str(DRIVER), str(src), "-L" + str(ROOT / "limbo_amd"),
                           "-lgpengine", "-Wl,-rpath,$ORIGIN/../../limbo_amd", "-Wl,-rpath,/opt/rocm/lib", "-lpthread"])
    return DRIVER


def dropin_problem(n, M, B, seed, D=6):
    """a smooth objective of x in [0, 1]^D, amplitude 0.3, observation noise 0.1; candidates in the box; the baseline: the B best
    observed points; SE-ARD with length scale 0.5"""
    rng = np.random.default_rng(seed)
    X = rng.random((n, D))
    Y = 0.3 * np.sin(3.0 * X @ rng.random(D)) + 0.1 * rng.standard_normal(n)
    Q = rng.random((M, D))
    Xb = X[np.argsort(-Y, kind="stable")[:B]]
    return X, Y[:, None], Q, Xb, np.log([0.5] * D + [1.0])


def run_driver(tmp_path, X, Y, Q, Xb, S, seed, hp, s_prune=16, env=None):
    exe = build_driver()
    n, D = X.shape
    f = tmp_path / "in.txt"
    with open(f, "w") as fh:
        fh.write(f"{D} {n} {len(Q)} {len(Xb)} {S} {seed} {len(hp)} {s_prune}\n")
        fh.write(" ".join(repr(float(v)) for v in hp) + "\n")
        for i in range(n):
            fh.write(" ".join(repr(float(v)) for v in list(X[i]) + list(Y[i])) + "\n")
        for v in list(Q) + list(Xb):
            fh.write(" ".join(repr(float(x)) for x in v) + "\n")
    r = subprocess.run([str(exe), str(f)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return {ln.split()[0]: np.array([float(v) for v in ln.split()[1:]]) for ln in r.stdout.splitlines()}


def check_dropin(got, X, Y, Q, Xb, S, hp, what):
    """the driver's numbers against ref_pipeline on the driver's own base normals: fplus, cmean and cvar at the parity bar 1e-8, lognei at
    the end-to-end bound of tests/test_gpu_nei.py (10 E_REF_NEI max(1, |ref|) + the 1e-8 bar pushed through the terms' partials) over
    the candidates with every |z_s| <= 10 and cvar >= 1e-4; the wrappers bitwise; the arg-max the reference's.  Returns lognei."""
    B, M = len(Xb), len(Q)
    Z = got["Z"].reshape(S, B).T
    mval = float(Y.mean())
    ref = R.ref_pipeline(O.SE_ARD, hp, DROPIN_NOISE, X, Y - mval, 0, Xb, np.full(B, mval), DROPIN_JITTER, Z, DROPIN_XI, Q, np.full(M, mval))
    v, cm = got["one"], got["cmean"].reshape(M, S).T
    e_f, e_m, e_v = (float(R.err(g, r).max()) for g, r in ((got["fplus"], ref["fplus"]), (cm, ref["cmean"]), (got["cvar"], ref["cvar"])))
    dm, ds = R.term_partials(ref["fplus"], DROPIN_XI, ref["cmean"], ref["sd"])
    with np.errstate(all="ignore"):
        z = (ref["cmean"] - ref["fplus"][:, None] - DROPIN_XI) / ref["sd"][None, :]
        bound = 10 * E_REF_NEI * np.maximum(1.0, np.abs(ref["lognei"])) + np.abs(dm).max(axis=0) * 1e-8 + np.abs(ds).max(axis=0) * 1e-8 / (2 * ref["sd"])
    keep = (ref["cvar"] >= 1e-4) & np.all(np.abs(z) <= 10, axis=0)
    d = np.abs(v - ref["lognei"])
    print(f"{what}: fplus {e_f:.3e}, cmean {e_m:.3e}, cvar {e_v:.3e}; lognei in [{v.min():.3e}, {v.max():.3e}], max error {d[keep].max():.3e}, "
          f"worst share of the bound {np.max(d[keep] / bound[keep]):.3e} over {keep.sum()} of {M}; singular: {got['singular']}")
    assert int(got["status"][0]) == 0 and keep.mean() >= 0.5
    assert max(e_f, e_m, e_v) <= 1e-8 and np.all(d[keep] <= bound[keep]) and np.all(np.isfinite(v))
    for k in ("batch", "acq"):
        assert np.array_equal(got[k], v), k
    assert got["single"][0] == v[0]
    assert int(got["best"][0]) == int(np.argmax(ref["lognei"])) == int(np.argmax(v)) and int(got["best_none"][0]) == -1
    rc, left = got["singular"]
    assert 0 <= rc <= 2 * B and left == 0.0, "every baseline point twice, no jitter: refused with nothing written, or factored (rounding decides)"
    return v


def check_baseline(got, X):
    """nei_baseline: a subset of the samples that holds the arg-max of the posterior mean, ascending, deterministic for a seed"""
    idx, again, other = (got[k].astype(int) for k in ("baseline_idx", "baseline_idx_again", "baseline_idx_other"))
    n, D = X.shape
    assert np.array_equal(idx, again), "deterministic for a seed"
    assert len(idx) >= 1 and np.all(np.diff(idx) > 0) and idx.min() >= 0 and idx.max() < n
    assert int(np.argmax(got["mu_train"])) in idx and int(np.argmax(got["mu_train"])) in other
    assert np.array_equal(got["baseline_pts"].reshape(-1, D), X[idx])
    return idx


def test_dropin_host_path(tmp_path):
    """n = 60 with the host switches: GP::log_noisy_ei through model/gp/nei.hpp, nothing touches the device"""
    S, seed = 7, 5
    X, Y, Q, Xb, hp = dropin_problem(60, 20, 9, 21)
    got = run_driver(tmp_path, X, Y, Q, Xb, S, seed, hp, env=HOST_ENV)
    assert int(got["host_resident"][0]) == 1
    check_dropin(got, X, Y, Q, Xb, S, hp, "host, n = 60")
    idx = check_baseline(got, X)
    print("baseline", idx)
    assert len(idx) <= 17, "at most S_prune arg-max points and the best mean"
