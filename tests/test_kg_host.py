"""The knowledge gradient over a finite alternative set (include/gpe_kg.h) — what can be held WITHOUT a device:

* the C-ABI: a header of its own (include/gpe.h declares none of it), exported by libgpengine.so, bound by limbo_amd._capi;
* the accuracy of the REFERENCE every other comparison leans on: tests/kg_ref.py's ref_h (the paper's sorted stack algorithm in
  double precision) against the same quantity in 50-digit arithmetic on about 40 small cases — random lines, concurrent lines, equal
  slopes, inputs on a coarse grid, breakpoints out to |z| = 35.  f(-|z|) = phi(z) - |z| Phi(-|z|) loses about z^2 ulps to
  cancellation at large |z| (and exp(-z^2 / 2) feels the rounding of z^2), so the error is MEASURED, not assumed: the worst relative
  error is the constant E_REF below, and the bars of the device tests (tests/test_gpu_kg.py) are multiples of it;
* the host path of the C++ drop-in (model::GP::knowledge_gradient, acqui/kg.hpp below Params::gpu::min_n_for_gpu, and the empty
  model): tests/cpp/test_kg_dropin, compiled here with the flags of tests/cpp/Makefile, against ref_kg on the beliefs the driver
  itself reports (equal inputs: what is compared is the envelope), and those beliefs against the CPU oracle's factor and alpha."""
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import scipy.linalg as sla

from limbo_amd import _capi
from oracle import np_oracle as O
from tests import kg_cases as K
from tests import kg_ref as R

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("gpe_kg_batch", "gpe_kg_envelope", "gpe_kg_phase_ms")
# worst relative error of ref_h against 50-digit arithmetic over kg_cases.small_cases(), measured 2026-10-20 (1.4211e-10, at the
# breakpoint |z| = 30.9; the cases with every |z| < 5 are below 6e-15)
E_REF = 1.43e-10


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_abi_lives_in_its_own_header(engine_lib):
    hs = (ROOT / "include" / "gpe_kg.h").read_text()
    h = (ROOT / "include" / "gpe.h").read_text()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hs), n + " is not declared in include/gpe_kg.h"
        assert not re.search(r"\b" + n + r"\s*\(", h), n + " must not be declared in include/gpe.h"
        assert hasattr(engine_lib.cdll, n), n + " is not exported by libgpengine.so"
        assert engine_lib.fn(n[4:]).argtypes is not None, n + " is not bound by _capi"
    assert '#include "gpe.h"' in hs
    for m in ("kg_batch", "kg_envelope", "kg_phase_ms"):
        assert callable(getattr(_capi.Handle, m))
    assert _capi.KG_MAX_ALTERNATIVES == 2048
    assert re.search(r"#define\s+GPE_KG_MAX_ALTERNATIVES\s+2048\b", hs)
    assert b"k_kg_envelope" in _capi.ENGINE_SO.read_bytes(), "the envelope kernel is in the shipped code object"


# ------------------------------------------------------------------------------------------------ the reference's own accuracy
def test_reference_against_50_digits():
    cases = K.small_cases()
    assert 35 <= len(cases) <= 45
    worst, zmax = 0.0, 0.0
    for name, a, b in cases:
        assert len(a) <= 64
        exact = R.mp_h(a, b)
        got = R.ref_h(a, b)
        assert exact > 0 and got >= 0
        err = float(abs(got - exact) / exact)
        print(f"{name:24s} h = {float(exact):.6e}  relative error {err:.3e}")
        worst = max(worst, err)
        if name.startswith("far"):
            zmax = max(zmax, abs(float(name.split("_")[1])))
    print(f"worst relative error {worst:.4e} (E_REF = {E_REF:.4e})")
    assert zmax >= 34.0, "breakpoints out to |z| = 35 are among the cases"
    assert worst <= E_REF


def test_reference_properties():
    """what the construction promises, on the reference: invariance to a shift of dyadic a (bitwise), zero for equal slopes, every
    tangent of a parabola on the envelope, and agreement with plain quadrature of E[max] - max where that does not cancel"""
    a, b = K.grid(64, 5)
    assert R.ref_h(a, b) == R.ref_h(a + 2.0 ** 20, b)
    assert R.ref_h(a, np.full(64, 0.75)) == 0.0 and R.ref_h(a, np.zeros(64)) == 0.0 and R.ref_h(a[:1], b[:1]) == 0.0
    pa, pb = K.parabola(65)
    assert R.ref_nseg(pa, pb) == 64
    z = np.linspace(-12.0, 12.0, 480001)
    w = np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)
    for A, seed in ((5, 3), (33, 4)):
        a, b = K.random_lines(A, seed)
        quad = getattr(np, "trapezoid", None) or np.trapz
        quad = quad(np.max(a[:, None] + b[:, None] * z[None, :], axis=0) * w, z) - a.max()
        assert abs(quad - R.ref_h(a, b)) <= 1e-9


# ------------------------------------------------------------------------------------------------ the drop-in's host path
DRIVER = ROOT / "tests" / "cpp" / "test_kg_dropin"
NOISES = (0.01, 0.1)  # Params::kernel::noise of the driver by noise_id


def build_driver():
    """tests/cpp/test_kg_dropin with the flags of tests/cpp/Makefile (that file is not this test's to change)"""
    src = DRIVER.with_suffix(".cpp")
    deps = [src, _capi.ENGINE_SO] + list((ROOT / "include").rglob("*.h*"))
    if DRIVER.exists() and all(DRIVER.stat().st_mtime >= d.stat().st_mtime for d in deps):
        return DRIVER
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Wno-unused-variable", "-I" + str(ROOT / "include" / "limbo_amd"),
                           "-I" + str(ROOT / "oracle" / "ref_build" / "shim"), "-o", str(DRIVER), str(src), "-L" + str(ROOT / "limbo_amd"),
                           "-lgpengine", "-Wl,-rpath,$ORIGIN/../../limbo_amd", "-Wl,-rpath,/opt/rocm/lib", "-lpthread"])
    return DRIVER


def run_driver(tmp_path, kind, mean, X, Y, Qa, Qc, agg, with_self, noise_id=0, hp=None, env=None):
    exe = build_driver()
    n, D = X.shape
    P = Y.shape[1]
    f = tmp_path / "in.txt"
    with open(f, "w") as fh:
        fh.write(f"{kind} {mean} {P} {D} {n} {len(Qa)} {len(Qc)} {agg} {int(with_self)} {noise_id} {0 if hp is None else len(hp)}\n")
        if hp is not None:
            fh.write(" ".join(repr(float(v)) for v in hp) + "\n")
        for i in range(n):
            fh.write(" ".join(repr(float(v)) for v in list(X[i]) + list(Y[i])) + "\n")
        for v in list(Qa) + list(Qc):
            fh.write(" ".join(repr(float(x)) for x in v) + "\n")
    r = subprocess.run([str(exe), str(f)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        out[w[0]] = np.array([float(v) for v in w[1:]])
    return out


def dropin_problem(kind, P, n, A, M, seed):
    D = 3 if kind == 0 else 2
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, size=(n, D))
    Y = np.stack([np.cos((p + 1.5) * X.sum(axis=1)) + 0.3 * X[:, 0] for p in range(P)], axis=1).reshape(n, P) + 0.05 * rng.normal(size=(n, P))
    return X, Y, rng.uniform(0, 1, size=(A, D)), rng.uniform(0, 1, size=(M, D))


def dropin_reference(oracle_lib, kind, mean, X, Y, Q, noise, th=None):
    """(Sig, mu (T x P, the mean functor added)) over the points Q from the CPU oracle's factor and alpha"""
    n, D = X.shape
    P = Y.shape[1]
    if th is None:
        th = np.zeros(D + 1) if kind == 0 else np.zeros(2)  # the functors' default hyper-parameters
    mval = (Y.mean(axis=0) if n else np.zeros(P)) if mean == 0 else np.ones(P)  # mean::Data / mean::Constant (constant 1)
    Sig = O.kernel_cross(kind, Q, Q, th)
    if n == 0:
        return Sig, np.tile(mval, (len(Q), 1))
    h = _capi.Handle(oracle_lib)
    h.set_data(X, Y - mval)
    h.set_kernel(kind, th, noise)
    assert h.compute() == 0
    L, al = h.get_L(), h.get_alpha()
    h.close()
    Ks = O.kernel_cross(kind, X, Q, th)
    Zs = sla.solve_triangular(L, Ks, lower=True)
    return Sig - Zs.T @ Zs, Ks.T @ al + mval


def rel_err(got, ref):
    """max relative difference where the reference is a normal number; elsewhere `got` must be as small"""
    big = ref >= 1e-280
    assert np.all(got >= 0) and np.all(got[~big] <= 1e-279)
    return float(np.max(np.abs(got[big] - ref[big]) / ref[big])) if big.any() else 0.0


# (kind, mean, P, n, agg, with_self): the prior; one sample; Matern-5/2 with the Data mean; two outputs with the second-element
# aggregator (complete means from query_batch), with and without the candidate among the alternatives
HOST_CASES = [(0, 0, 1, 0, 0, 1), (0, 0, 1, 1, 0, 1), (1, 0, 1, 40, 0, 0), (0, 0, 2, 200, 1, 1), (0, 2, 2, 200, 1, 0)]


@pytest.mark.parametrize("kind,mean,P,n,agg,with_self", HOST_CASES)
def test_dropin_host_path(tmp_path, oracle_lib, kind, mean, P, n, agg, with_self):
    A, M = 24, 40
    X, Y, Qa, Qc = dropin_problem(kind, P, n, A, M, 1000 * kind + 100 * mean + 10 * P + n)
    got = run_driver(tmp_path, kind, mean, X, Y, Qa, Qc, agg, with_self,
                     env={"LIMBO_AMD_MIN_N_FOR_GPU": str(1 << 20), "LIMBO_AMD_HOST_BATCH_CROSSOVER": str(1 << 40)})
    assert n == 0 or got["host_resident"][0] == 1
    T = A + M
    mu, cov = got["mu"].reshape(T, P, order="F"), got["cov"].reshape(T, T, order="F")
    # the beliefs the driver worked from are the oracle's
    Sig, mu_o = dropin_reference(oracle_lib, kind, mean, X, Y, np.vstack([Qa, Qc]), NOISES[0])
    assert np.max(np.abs(cov - Sig)) <= 1e-8 and np.max(np.abs(mu - mu_o)) <= 1e-8
    # the envelope, given equal inputs
    ref = R.ref_kg(cov, mu[:, agg], np.arange(A), A + np.arange(M), NOISES[0], bool(with_self))
    e = rel_err(got["kg"], ref)
    print(f"kg in [{ref.min():.3e}, {ref.max():.3e}], max relative error {e:.3e}")
    assert e <= 10 * E_REF
    assert int(got["best"][0]) == int(np.argmax(ref)) == int(np.argmax(got["kg"]))
    # no means passed: k^T alpha of output 0 — the mean functor taken off again (a constant: it moves nothing)
    ref0 = R.ref_kg(cov, mu[:, 0], np.arange(A), A + np.arange(M), NOISES[0], bool(with_self))
    assert rel_err(got["plain"], ref0) <= 10 * E_REF
    if n == 0:  # the prior: every mean equal — only the candidate's own line can rise above the others
        assert np.all(got["kg"] > 0) if with_self else np.all(got["kg"] >= 0)
