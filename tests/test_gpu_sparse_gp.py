"""The sparse pseudo-input GP on the device (include/gpe_sparse.h): parity, summation order, reproducibility, the contract, and the
C++ drop-in limbo::model::SPGP.

The checker is never the engine: tests/sparse_ref.py, route (a) = the reference's own sequence (spgp.hpp:394-406, 491, 597-608) in
numpy / LAPACK; its agreement with the dense definition, route (b), is held to a thousandth of the bars below by
tests/test_sparse_host.py.  Bars: 1e-8 absolute on mu and s2 (sigma_f = 1, |y| ~ 1), 1e-10 relative on the
likelihood; ep at 1e-8.  Inputs: tests/sparse_ref.make_problem (X uniform in [0, 1]^D, pseudo-inputs a random subset, y = sin(3 X.u)
+ 0.1 N(0, 1) centred, c = 1, sig = 0.01, length scales 0.3 .. 1.0), jitter 1e-6 and 1e-4.

Shapes (N, M, D, P): M below one 256-column outer panel (the N x M layout: 40, 193) and above it (the transposed layout: 256, 320,
1024), M no multiple of 64 (40, 193), the 64 x 64 and the 128 x 128 tile of the solve (M < 1024 / = 1024), D > 16, P = 2; each with
GPE_SPARSE_CHUNK=512 (several chunks, a ragged last one) and with the default chunk (one chunk at these N)."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from limbo_amd import _capi
from tests import sparse_ref as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CASES = [(1300, 40, 3, 1), (1300, 193, 6, 2), (1500, 320, 6, 1), (5000, 1024, 6, 1), (1500, 256, 20, 1)]
IDS = ["n%d_m%d_d%d_p%d" % c for c in CASES]
JITTERS = [1e-6, 1e-4]
BAR_ABS, BAR_LIK, BAR_ORDER = 1e-8, 1e-10, 1e-10
_cache = {}


def problem(case):
    if case not in _cache:
        _cache[case] = (R.make_problem(*case, seed=31 + CASES.index(case)), {})
    return _cache[case]


def reference(case, jitter):
    pr, refs = problem(case)
    if jitter not in refs:
        refs[jitter] = R.route_a(pr["X"], pr["Xb"], pr["y"], pr["log_b"], pr["log_c"], pr["log_sig"], jitter, pr["Xt"])
    return pr, refs[jitter]


def fit(lib, pr, jitter):
    h = _capi.SparseHandle(lib)
    h.set_data(pr["X"], pr["y"])
    h.set_pseudo(pr["Xb"])
    h.set_hparams(pr["log_b"], pr["log_c"], pr["log_sig"], jitter)
    assert h.compute() == 0
    return h


def answers(h, pr):
    mu, s2 = h.predict(pr["Xt"])
    return dict(mu=mu, s2=s2, nlml=h.nlml(), ep=h.get_ep(), bet=h.get_bet())


def run(lib, pr, jitter, chunk, monkeypatch):
    if chunk:
        monkeypatch.setenv("GPE_SPARSE_CHUNK", str(chunk))  # (read by the library per call)
    else:
        monkeypatch.delenv("GPE_SPARSE_CHUNK", raising=False)
    h = fit(lib, pr, jitter)
    out = answers(h, pr)
    h.close()
    return out


@pytest.mark.parametrize("jitter", JITTERS)
@pytest.mark.parametrize("chunk", [512, 0], ids=["chunk512", "chunk_default"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_parity_with_the_reference_sequence(engine_lib, monkeypatch, case, chunk, jitter):
    pr, ref = reference(case, jitter)
    got = run(engine_lib, pr, jitter, chunk, monkeypatch)
    d_mu = np.max(np.abs(got["mu"] - ref["mu"]))
    d_s2 = np.max(np.abs(got["s2"] - ref["s2"]))
    d_ep = np.max(np.abs(got["ep"] - ref["ep"]))
    d_lik = np.max(np.abs(got["nlml"] - ref["nlml"]) / np.abs(ref["nlml"]))
    print(f"{case} chunk={chunk} jitter={jitter:g}: |mu - a| = {d_mu:.3e}  |s2 - a| = {d_s2:.3e}  |ep - a| = {d_ep:.3e}  "
          f"nlml rel = {d_lik:.3e}  (nlml = {got['nlml']})")
    assert d_mu <= BAR_ABS
    assert d_s2 <= BAR_ABS
    assert d_ep <= BAR_ABS
    assert d_lik <= BAR_LIK


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_chunk_lengths_agree_and_calls_repeat_bitwise(engine_lib, monkeypatch, case):
    """Another chunk length is another summation order: agreement to 1e-10, no bitwise claim.  The same call twice IS bitwise
    equal, and so are 400 points asked at once and 100 at a time."""
    pr, _ = problem(case)
    a = run(engine_lib, pr, 1e-6, 512, monkeypatch)
    b = run(engine_lib, pr, 1e-6, 0, monkeypatch)
    d_mu, d_s2 = np.max(np.abs(a["mu"] - b["mu"])), np.max(np.abs(a["s2"] - b["s2"]))
    d_lik = np.max(np.abs(a["nlml"] - b["nlml"]) / np.abs(b["nlml"]))
    print(f"{case}: chunk 512 against the default: |mu| {d_mu:.3e}  |s2| {d_s2:.3e}  nlml rel {d_lik:.3e}")
    assert d_mu <= BAR_ORDER and d_s2 <= BAR_ORDER and d_lik <= BAR_ORDER
    for chunk, first in ((512, a), (0, b)):
        again = run(engine_lib, pr, 1e-6, chunk, monkeypatch)
        for k in first:
            assert np.array_equal(first[k], again[k]), (chunk, k)
    h = fit(engine_lib, pr, 1e-6)
    mu, s2 = h.predict(pr["Xt"])
    for t0 in range(0, 400, 100):
        m, s = h.predict(pr["Xt"][t0:t0 + 100])
        assert np.array_equal(m, mu[t0:t0 + 100]) and np.array_equal(s, s2[t0:t0 + 100]), t0
    m1, _ = h.predict(pr["Xt"], want_s2=False)
    _, s1 = h.predict(pr["Xt"], want_mu=False)
    assert np.array_equal(m1, mu) and np.array_equal(s1, s2)
    h.close()


@pytest.mark.parametrize("gram", ["0", "1"])
def test_gram_switch_both_paths_meet_the_bars(engine_lib, monkeypatch, gram):
    """GPE_SPARSE_GRAM=0: the composed path (a weighted copy of V through the engine's general product) stays in the tree — and is
    the default from 512 lower tiles on; 1 forces the kernel"""
    monkeypatch.setenv("GPE_SPARSE_GRAM", gram)
    # (chunks of 256 columns are one slice each: the kernel then adds into A itself, without partial matrices and a fold)
    for case, chunk in ((CASES[1], 512), (CASES[2], 512), (CASES[2], 256)):
        pr, ref = reference(case, 1e-6)
        got = run(engine_lib, pr, 1e-6, chunk, monkeypatch)
        d = (np.max(np.abs(got["mu"] - ref["mu"])), np.max(np.abs(got["s2"] - ref["s2"])),
             np.max(np.abs(got["nlml"] - ref["nlml"]) / np.abs(ref["nlml"])))
        print(f"GPE_SPARSE_GRAM={gram} {case} chunk={chunk}: |mu| {d[0]:.3e} |s2| {d[1]:.3e} nlml rel {d[2]:.3e}")
        assert d[0] <= BAR_ABS and d[1] <= BAR_ABS and d[2] <= BAR_LIK


def test_status_codes(engine_lib, monkeypatch):
    monkeypatch.delenv("GPE_SPARSE_CHUNK", raising=False)
    pr, _ = problem(CASES[0])
    X, y, Xb = pr["X"], pr["y"], pr["Xb"]
    hp = (pr["log_b"], pr["log_c"], pr["log_sig"])
    h = _capi.SparseHandle(engine_lib)
    assert h.compute(check=False) == -2                      # nothing set
    assert h.set_pseudo(Xb, check=False) == -2               # D comes from the data
    assert h.set_hparams(*hp, 1e-6, check=False) == -2
    assert h.set_data(X[:0], y[:0], check=False) == -1       # N < 1
    assert h.set_data(X, y) == 0
    assert h.compute(check=False) == -2                      # no pseudo-inputs, no hyper-parameters
    assert h.set_pseudo(Xb[:0], check=False) == -1           # M < 1
    assert h.set_pseudo(np.vstack([X, X[:1]]), check=False) == -1  # M > N
    assert h.set_pseudo(Xb) == 0
    assert h.compute(check=False) == -2                      # no hyper-parameters
    assert h.set_hparams(*hp, 0.99e-8, check=False) == -1    # jitter below 1e-8
    assert h.set_hparams(*hp, float("nan"), check=False) == -1
    assert h.set_hparams(hp[0], float("inf"), hp[2], 1e-6, check=False) == -1
    assert h.compute(check=False) == -2                      # ... and none of those was taken
    out = np.zeros(1)
    assert engine_lib.fn("sp_nlml")(h._h, _capi._d(out)) == -2
    assert engine_lib.fn("sp_predict")(h._h, _capi._d(np.ascontiguousarray(pr["Xt"])), 4, None, _capi._d(np.zeros(4))) == -2
    assert h.set_hparams(*hp, 1e-6) == 0
    assert h.compute() == 0
    assert engine_lib.fn("sp_predict")(h._h, None, 4, None, _capi._d(np.zeros(4))) == -1
    # a setter invalidates the model
    assert h.set_hparams(*hp, 1e-4) == 0
    assert engine_lib.fn("sp_nlml")(h._h, _capi._d(out)) == -2
    # sig = exp(-800) = 0: w = 1 / ep = 0 for every point and A = 0 I + 0 is the zero matrix — its first pivot fails: M + 1
    assert h.set_hparams(hp[0], hp[1], -800.0, 1e-6) == 0
    assert h.compute() == pr["M"] + 1
    assert engine_lib.fn("sp_nlml")(h._h, _capi._d(out)) == -2
    h.close()


def test_m_equal_n_and_a_duplicated_pseudo_input(engine_lib, monkeypatch):
    monkeypatch.delenv("GPE_SPARSE_CHUNK", raising=False)
    pr = R.make_problem(300, 300, 6, 1, seed=5)
    pr["Xb"] = pr["X"].copy()  # M = N: every point its own pseudo-input
    ref = R.route_a(pr["X"], pr["Xb"], pr["y"], pr["log_b"], pr["log_c"], pr["log_sig"], 1e-6, pr["Xt"])
    h = fit(engine_lib, pr, 1e-6)
    got = answers(h, pr)
    h.close()
    d = (np.max(np.abs(got["mu"] - ref["mu"])), np.max(np.abs(got["s2"] - ref["s2"])), np.max(np.abs(got["nlml"] - ref["nlml"]) / np.abs(ref["nlml"])))
    print(f"M = N = 300: |mu| {d[0]:.3e} |s2| {d[1]:.3e} nlml rel {d[2]:.3e}")
    assert d[0] <= BAR_ABS and d[1] <= BAR_ABS and d[2] <= BAR_LIK
    pr2, _ = problem(CASES[1])
    dup = dict(pr2)
    dup["Xb"] = pr2["Xb"].copy()
    dup["Xb"][7] = dup["Xb"][3]  # K(Xb, Xb) is singular without the jitter
    h = fit(engine_lib, dup, 1e-6)  # asserts status 0
    mu, s2 = h.predict(dup["Xt"])
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(s2))
    h.close()


def test_rewritten_hyper_parameters_equal_a_fresh_handle(engine_lib, monkeypatch):
    monkeypatch.setenv("GPE_SPARSE_CHUNK", "512")
    for case in (CASES[0], CASES[2]):
        pr, _ = problem(case)
        h = fit(engine_lib, pr, 1e-4)
        rc, lik = h.objective(pr["log_b"] + 0.1, pr["log_c"] - 0.2, pr["log_sig"] + 0.3, 1e-6)
        assert rc == 0
        used = answers(h, pr)
        h.close()
        fresh = _capi.SparseHandle(engine_lib)
        fresh.set_data(pr["X"], pr["y"])
        fresh.set_pseudo(pr["Xb"])
        fresh.set_hparams(pr["log_b"] + 0.1, pr["log_c"] - 0.2, pr["log_sig"] + 0.3, 1e-6)
        assert fresh.compute() == 0
        new = answers(fresh, pr)
        L, Lm = fresh.get_L(), fresh.get_Lm()
        fresh.close()
        assert np.array_equal(lik, new["nlml"])
        for k in used:
            assert np.array_equal(used[k], new[k]), k
        assert np.all(np.triu(L, 1) == 0) and np.all(np.triu(Lm, 1) == 0) and np.all(np.diag(L) > 0) and np.all(np.diag(Lm) > 0)


# ---- the C++ drop-in: include/limbo_amd/limbo/experimental/model/spgp.hpp ---------------------------------------------------------
DRIVER = ROOT / "tests" / "cpp" / "test_spgp"


def build_driver():
    """tests/cpp/test_spgp with the flags of tests/cpp/Makefile (which this change leaves alone)"""
    src = DRIVER.with_suffix(".cpp")
    deps = [src, ROOT / "limbo_amd" / "libgpengine.so", ROOT / "include" / "gpe_sparse.h",
            ROOT / "include" / "limbo_amd" / "limbo" / "experimental" / "model" / "spgp.hpp"]
    if DRIVER.exists() and all(DRIVER.stat().st_mtime >= d.stat().st_mtime for d in deps):
        return DRIVER
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-Wall", "-Wno-unused-variable", f"-I{ROOT}/include/limbo_amd",
           f"-I{ROOT}/oracle/ref_build/shim", "-o", str(DRIVER), str(src), f"-L{ROOT}/limbo_amd", "-lgpengine",
           "-Wl,-rpath,$ORIGIN/../../limbo_amd", "-Wl,-rpath,/opt/rocm/lib", "-lpthread"]
    subprocess.check_call(cmd)
    return DRIVER


def test_cpp_dropin(tmp_path):
    """A pinned model (set_pseudo_samples + set_h_params) predicts within 1e-8 of route (a), which this test writes to a file;
    optimize_hyperparams() does not raise the nlml; add_sample followed by query works."""
    drv = build_driver()
    pr = R.make_problem(1300, 130, 3, 1, seed=3, T=64)
    ref = R.route_a(pr["X"], pr["Xb"], pr["y"], pr["log_b"], pr["log_c"], pr["log_sig"], 1e-6, pr["Xt"])
    f = tmp_path / "spgp_case.txt"
    with open(f, "w") as o:
        o.write(f"{pr['N']} {pr['M']} {pr['D']} {pr['Xt'].shape[0]}\n")
        for name in ("X", "Xb", "Xt"):
            o.write(" ".join(repr(float(v)) for v in pr[name].ravel()) + "\n")
        o.write(" ".join(repr(float(v)) for v in pr["y"][:, 0]) + "\n")
        o.write(" ".join(repr(float(v)) for v in pr["log_b"]) + f" {pr['log_c']!r} {float(pr['log_sig'])!r}\n")
        o.write(" ".join(repr(float(v)) for v in ref["mu"][:, 0]) + "\n")
        o.write(" ".join(repr(float(v)) for v in ref["s2"]) + "\n")
        o.write(repr(float(ref["nlml"][0])) + "\n")
    r = subprocess.run([str(drv), str(f)], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
