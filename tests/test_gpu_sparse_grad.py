"""The sparse pseudo-input GP's analytic gradient on the device (include/gpe_sparse_grad.h) against the two references of
tests/sparse_grad_ref.py — the reference's own sequence (spgp.hpp:453-580, P = 1) and autograd of the dense FITC definition (any
P, N <= 1500) — and its contract: reproducibility, what it leaves untouched, the statuses, the tie to gpe_sp_objective, and the C++
drop-in's fit (tests/cpp/test_spgp_grad.cpp).

The bar is the project's gradient bar: 1e-6 per block — d_xb; d log b; {d log c, d log sig} — the error of a block being
max |a - b| / max |b| over it.  The references agree with each other to <= 2e-11 (tests/test_sparse_grad_host.py), the same form in
numpy with explicit inverses sits at <= 4.3e-9 of them: the bar leaves about 200 x for the order of the sums.

The shapes are the smallest that reach each path: M below one 64-tile and one outer panel with P = 3; a ragged tile with P = 2; two
outer panels and a ragged one; exactly one panel with D > 16 (41 row sums, three column groups); M = 1024 (several panels).  Each
with GPE_SPARSE_CHUNK=512 (several chunks, a ragged last one) and the default chunk.

Measured on an MI355X when this was written (worst block over both jitters and both chunkings): (700, 40, 3, 3) and
(1300, 193, 6, 2) <= 3e-11, (1500, 320, 6, 1) 2.8e-11 against either route, (900, 256, 20, 1) 4.0e-14, (5000, 1024, 6, 1) 2.7e-9;
chunk 512 against the default chunk 5.4e-12 and 1.5e-11; the central difference 3.7e-8."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from limbo_amd import _capi
from tests import sparse_grad_ref as G
from tests import sparse_ref as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CASES = [(700, 40, 3, 3), (1300, 193, 6, 2), (1500, 320, 6, 1), (900, 256, 20, 1), (5000, 1024, 6, 1)]
IDS = ["n%d_m%d_d%d_p%d" % c for c in CASES]
ROUTES = {CASES[0]: ("autograd",), CASES[1]: ("autograd",), CASES[2]: ("autograd", "sequence"), CASES[3]: ("autograd",), CASES[4]: ("sequence",)}
RUNS = [(c, j) for c in CASES for j in ((1e-6, 1e-4) if c in CASES[:3] else (1e-6,))]
BAR, BAR_ORDER, BAR_FD = 1e-6, 1e-9, 1e-5
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def engine_first(engine_lib):
    """The engine brings the HIP runtime up before tests/sparse_grad_ref.py imports torch for its CPU autograd: in a process
    where torch came first, creating a handle failed with GPE_ERR_HIP (seen when this file was written)."""
    _capi.SparseHandle(engine_lib).close()


def problem(case):
    if case not in _cache:
        pr = R.make_problem(*case, seed=41 + CASES.index(case), T=64)
        pr["Xb"] = G.off_the_data(pr)  # (the subset itself is a special point: the pseudo-inputs sit off the data)
        _cache[case] = (pr, {})
    return _cache[case]


def references(case, jitter):
    pr, refs = problem(case)
    if jitter not in refs:
        args = (pr["X"], pr["Xb"], pr["y"], pr["log_b"], pr["log_c"], pr["log_sig"], jitter)
        refs[jitter] = {r: (G.autograd_grad if r == "autograd" else G.ref_grad)(*args) for r in ROUTES[case]}
    return pr, refs[jitter]


def set_chunk(monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv("GPE_SPARSE_CHUNK", str(chunk))  # (read by the library per call)
    else:
        monkeypatch.delenv("GPE_SPARSE_CHUNK", raising=False)


def fit(lib, pr, jitter):
    h = _capi.SparseHandle(lib)
    h.set_data(pr["X"], pr["y"])
    h.set_pseudo(pr["Xb"])
    h.set_hparams(pr["log_b"], pr["log_c"], pr["log_sig"], jitter)
    assert h.compute() == 0
    return h


def as_route(f, gx, gh, D):
    return (float(np.sum(f)), gx, gh[:D], gh[D], gh[D + 1])


def device_grad(lib, pr, jitter):
    h = fit(lib, pr, jitter)
    f = h.nlml()
    rc, gx, gh = h.grad()
    h.close()
    assert rc == 0
    return as_route(f, gx, gh, pr["D"])


@pytest.mark.parametrize("chunk", [512, 0], ids=["chunk512", "chunk_default"])
@pytest.mark.parametrize("case,jitter", RUNS, ids=["%s_j%g" % (IDS[CASES.index(c)], j) for c, j in RUNS])
def test_gradient_against_the_references(engine_lib, monkeypatch, case, jitter, chunk):
    pr, refs = references(case, jitter)
    set_chunk(monkeypatch, chunk)
    got = device_grad(engine_lib, pr, jitter)
    for route, ref in refs.items():
        err = G.block_errors(got, ref)
        print(f"{case} chunk={chunk} jitter={jitter:g} against {route}: F {got[0]:.9f} / {ref[0]:.9f}  " + "  ".join(f"{k} {v:.3e}" for k, v in err.items()))
        assert abs(got[0] - ref[0]) <= 1e-9 * abs(ref[0])
        for k, v in err.items():
            assert v <= BAR, (route, k)


@pytest.mark.parametrize("gram", ["0", "1"])
def test_gram_switch_both_paths_meet_the_bar(engine_lib, monkeypatch, gram):
    """TT by the composed path (=0) and by the split-k kernel (=1), whose weights are signed here"""
    case = CASES[2]
    pr, refs = references(case, 1e-6)
    monkeypatch.setenv("GPE_SPARSE_GRAM", gram)
    for chunk in (512, 0):
        set_chunk(monkeypatch, chunk)
        got = device_grad(engine_lib, pr, 1e-6)
        for route, ref in refs.items():
            err = G.block_errors(got, ref)
            print(f"GPE_SPARSE_GRAM={gram} {case} chunk={chunk} against {route}: " + "  ".join(f"{k} {v:.3e}" for k, v in err.items()))
            assert max(err.values()) <= BAR


@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=[IDS[0], IDS[2]])
def test_calls_repeat_bitwise_and_chunk_lengths_agree(engine_lib, monkeypatch, case):
    pr, _ = problem(case)
    out = {}
    for chunk in (512, 0):
        set_chunk(monkeypatch, chunk)
        h = fit(engine_lib, pr, 1e-6)
        f = h.nlml()
        rc1, gx1, gh1 = h.grad()
        rc2, gx2, gh2 = h.grad()
        h.close()
        assert rc1 == 0 and rc2 == 0
        assert np.array_equal(gx1, gx2) and np.array_equal(gh1, gh2)
        out[chunk] = as_route(f, gx1, gh1, pr["D"])
    err = G.block_errors(out[512], out[0])
    print(f"{case}: chunk 512 against the default: " + "  ".join(f"{k} {v:.3e}" for k, v in err.items()))
    assert max(err.values()) <= BAR_ORDER


def test_grad_leaves_the_model_as_it_was(engine_lib, monkeypatch):
    set_chunk(monkeypatch, 512)
    for case in (CASES[0], CASES[2]):
        pr, _ = problem(case)
        h = fit(engine_lib, pr, 1e-6)
        h.set_profiling(True)
        before = (h.nlml(), *h.predict(pr["Xt"]), h.get_bet(), h.get_ep())
        rc, gx, gh = h.grad()
        assert rc == 0 and np.all(np.isfinite(gx)) and np.all(np.isfinite(gh))
        ms = h.grad_phase_ms()
        print(case, "phases (ms):", ms)
        assert all(v >= 0.0 for v in ms.values()) and sum(ms.values()) > 0.0
        after = (h.nlml(), *h.predict(pr["Xt"]), h.get_bet(), h.get_ep())
        rc, gx2, gh2 = h.grad(want_xb=False)
        assert rc == 0 and gx2 is None and np.array_equal(gh, gh2)
        h.close()
        for a, b in zip(before, after):
            assert np.array_equal(a, b)


def test_objective_grad_on_a_used_handle_equals_a_fresh_one(engine_lib, monkeypatch):
    set_chunk(monkeypatch, 512)
    for case in (CASES[0], CASES[2]):
        pr, _ = problem(case)
        Xb2 = pr["Xb"] + 0.01
        hp2 = (pr["log_b"] + 0.1, pr["log_c"] - 0.2, pr["log_sig"] + 0.3)
        h = fit(engine_lib, pr, 1e-4)
        h.grad()
        rc, f, gx, gh = h.objective_grad(Xb2, *hp2, 1e-6)
        mu, s2 = h.predict(pr["Xt"])
        rck, fk, gxk, ghk = h.objective_grad(None, *hp2, 1e-6)  # (the pseudo-inputs kept)
        h.close()
        fresh = _capi.SparseHandle(engine_lib)
        fresh.set_data(pr["X"], pr["y"])
        fresh.set_pseudo(Xb2)
        fresh.set_hparams(*hp2, 1e-6)
        assert fresh.compute() == 0
        f0 = fresh.nlml()
        rc0, gx0, gh0 = fresh.grad()
        mu0, s20 = fresh.predict(pr["Xt"])
        fresh.close()
        assert rc == 0 and rc0 == 0 and rck == 0
        for a, b in ((f, f0), (gx, gx0), (gh, gh0), (mu, mu0), (s2, s20), (fk, f0), (gxk, gx0), (ghk, gh0)):
            assert np.array_equal(a, b)


def test_status_codes(engine_lib, monkeypatch):
    set_chunk(monkeypatch, 0)
    pr, _ = problem(CASES[0])
    hp = (pr["log_b"], pr["log_c"], pr["log_sig"])
    h = _capi.SparseHandle(engine_lib)
    assert h.grad(check=False)[0] == -2                                  # GPE_ERR_STATE: nothing set
    h.set_data(pr["X"], pr["y"])
    h.M = pr["M"]
    assert h.objective_grad(pr["Xb"], *hp, 1e-6, check=False)[0] == -2   # the handle has no M yet
    h.set_pseudo(pr["Xb"])
    h.set_hparams(*hp, 1e-6)
    assert h.grad(check=False)[0] == -2                                  # set, not computed
    assert h.compute() == 0
    assert h.grad()[0] == 0
    h.set_hparams(*hp, 1e-4)                                             # a setter invalidates the model
    assert h.grad(check=False)[0] == -2
    assert h.objective_grad(None, *hp, 0.99e-8, check=False)[0] == -1    # jitter below 1e-8
    # sig = exp(-800) = 0: A is the zero matrix and its first pivot fails (tests/test_gpu_sparse_gp.py): the status is the model's,
    # and nothing is written
    rc, f, gx, gh = h.objective_grad(None, hp[0], hp[1], -800.0, 1e-6)
    assert rc == pr["M"] + 1
    assert np.all(np.isnan(f)) and np.all(np.isnan(gx)) and np.all(np.isnan(gh))
    assert h.grad(check=False)[0] == -2
    rc, f, gx, gh = h.objective_grad(None, *hp, 1e-6)
    assert rc == 0 and np.all(np.isfinite(f)) and np.all(np.isfinite(gx)) and np.all(np.isfinite(gh))
    h.close()


def test_central_difference_of_the_objective(engine_lib, monkeypatch):
    """what the drop-in did before: central differences (h = 1e-5) of gpe_sp_objective in the D + 2 log-parameters"""
    set_chunk(monkeypatch, 0)
    pr, _ = problem(CASES[0])
    D = pr["D"]
    h = fit(engine_lib, pr, 1e-6)
    rc, _, gh = h.grad(want_xb=False)
    assert rc == 0
    w0 = np.r_[pr["log_b"], pr["log_c"], pr["log_sig"]]
    fd = np.zeros(D + 2)
    step = 1e-5
    for j in range(D + 2):
        v = []
        for s in (step, -step):
            w = w0.copy()
            w[j] += s
            rc, f = h.objective(w[:D], w[D], w[D + 1], 1e-6)
            assert rc == 0
            v.append(f.sum())
        fd[j] = (v[0] - v[1]) / (2 * step)
    h.close()
    e_b = np.max(np.abs(gh[:D] - fd[:D])) / np.max(np.abs(fd[:D]))
    e_cs = np.max(np.abs(gh[D:] - fd[D:])) / np.max(np.abs(fd[D:]))
    print(f"central difference: d log b {e_b:.3e}  d log c, sig {e_cs:.3e}  (analytic {gh}, difference {fd})")
    assert e_b <= BAR_FD and e_cs <= BAR_FD


# ---- the C++ drop-in's fit -------------------------------------------------------------------------------------------------------
DRIVER = ROOT / "tests" / "cpp" / "test_spgp_grad"


def build_driver():
    """tests/cpp/test_spgp_grad with the flags of tests/test_gpu_sparse_gp.py::build_driver (tests/cpp/Makefile stays as it is)"""
    src = DRIVER.with_suffix(".cpp")
    deps = [src, ROOT / "limbo_amd" / "libgpengine.so", ROOT / "include" / "gpe_sparse.h", ROOT / "include" / "gpe_sparse_grad.h",
            ROOT / "include" / "limbo_amd" / "limbo" / "experimental" / "model" / "spgp.hpp"]
    if DRIVER.exists() and all(DRIVER.stat().st_mtime >= d.stat().st_mtime for d in deps):
        return DRIVER
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-Wall", "-Wno-unused-variable", f"-I{ROOT}/include/limbo_amd",
           f"-I{ROOT}/oracle/ref_build/shim", "-o", str(DRIVER), str(src), f"-L{ROOT}/limbo_amd", "-lgpengine",
           "-Wl,-rpath,$ORIGIN/../../limbo_amd", "-Wl,-rpath,/opt/rocm/lib", "-lpthread"]
    subprocess.check_call(cmd)
    return DRIVER


def test_cpp_dropin_fit(tmp_path):
    """default Params: the fit does not raise the nlml and the pseudo-inputs stay the chosen subset bit for bit; with
    optimize_pseudo_inputs() the nlml does not rise, M is unchanged, a pseudo-input has moved, predictions are finite, s2 > 0"""
    drv = build_driver()
    pr = R.make_problem(1300, 130, 3, 1, seed=3, T=4)
    f = tmp_path / "spgp_grad_case.txt"
    with open(f, "w") as o:
        o.write(f"{pr['N']} {pr['M']} {pr['D']}\n")
        o.write(" ".join(repr(float(v)) for v in pr["X"].ravel()) + "\n")
        o.write(" ".join(repr(float(v)) for v in pr["y"][:, 0]) + "\n")
        o.write(" ".join(repr(float(v)) for v in pr["log_b"]) + f" {pr['log_c']!r} {float(pr['log_sig'])!r}\n")
    r = subprocess.run([str(drv), str(f)], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
