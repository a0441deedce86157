"""gpe_remove_samples (include/gpe_remove.h) without a GPU: the ABI (a header of its own, exported by libgpengine.so, bound by
limbo_amd._capi, absent from gpe.h), the numpy column sweep of tests/remove_ref.py against the refactorisation, the plan behind
GPE_REMOVE_AUTO (gpe_debug_remove_plan, host only), and the host path of the C++ drop-in's model::GP::remove_samples /
MultiGP::remove_samples / add_sample_windowed (tests/cpp/test_remove_samples, compiled here with the flags of tests/cpp/Makefile)
against a fresh compute() on the remaining samples."""
import ctypes
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from limbo_amd import _capi
from tests import remove_ref as RR
from tests.test_add_samples_host import _declared

ROOT = Path(__file__).resolve().parent.parent
DRIVER = ROOT / "tests" / "cpp" / "test_remove_samples"
SYMBOLS = {"gpe_remove_samples", "gpe_remove_max_vectors", "gpe_debug_remove_plan"}


def test_remove_header_declares_the_calls_and_gpe_h_does_not():
    assert SYMBOLS <= _declared("gpe_remove.h")
    assert not (SYMBOLS & _declared("gpe.h")) and not (SYMBOLS & _declared("gpe_append.h"))


def test_library_exports_and_binding():
    raw = ctypes.CDLL(str(_capi.ENGINE_SO))  # the dynamic symbol table itself, not the binding's view of it
    assert all(hasattr(raw, s) for s in SYMBOLS)
    lib = _capi.load_engine()
    assert len(lib.fn("remove_samples").argtypes) == 6 and len(lib.fn("debug_remove_plan").argtypes) == 5
    assert 1 <= _capi.remove_max_vectors(lib) <= 64  # host only: no device is touched
    assert hasattr(_capi.Handle, "remove_samples")
    assert (_capi.REMOVE_AUTO, _capi.REMOVE_UPDATE, _capi.REMOVE_RECOMPUTE) == (0, 1, 2)


# six shapes of the sweep (first, scattered with neighbours and the last, a run, every 11th, a larger order, an ill-conditioned one):
# (n, R, noise, bound on max |dL| / max |L|)
SWEEP_ROWS = [(700, [0], 0.01, 1e-12), (700, [5, 64, 65, 300, 699], 0.01, 1e-12), (700, list(range(100, 132)), 0.01, 1e-12),
              (700, list(range(0, 700, 11)), 0.01, 1e-12), (1500, [0, 1, 2, 700], 0.01, 1e-12),
              # noise 1e-6, condition 4e8: the bound is the condition number times the rounding of the sweep (4e8 * 1e-16 * a few)
              (700, [0, 350], 1e-6, 1e-9)]


@pytest.mark.parametrize("n,R,noise,tol", SWEEP_ROWS)
def test_numpy_sweep_equals_the_refactorisation(n, R, noise, tol):
    X = np.random.default_rng(n + len(R)).uniform(0, 1, size=(n, 6))
    K = RR.se_ard_kernel(X, noise)
    L = np.linalg.cholesky(K)
    got, want = RR.remove(L, R), RR.refactor(K, R)
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print(f"n {n} |R| {len(R)} noise {noise}: L {err:.2e}")
    assert got.shape == (n - len(R),) * 2 and np.all(np.diag(got) > 0) and err <= tol, err


def test_remove_plan():
    lib = _capi.load_engine()
    cap = _capi.remove_max_vectors(lib)
    plan = lambda *a: _capi.debug_remove_plan(lib, *a)
    # tail only: nothing is launched on the factor, whatever q is
    for n, q in ((300, 1), (300, 7), (16384, 16), (5000, 3 * cap)):
        path, passes, launches, scratch = plan(n, n - q, q, True)
        assert (path, passes, launches) == (1, 0, 0) and scratch > 0
    # passes = ceil(q / max_vectors); launches: per pass the head (if the first panel is not panel 0) and two per panel but the last
    for n, i0, q in ((600, 70, 1), (600, 70, cap), (600, 70, cap + 1), (700, 0, 64), (5000, 1000, 3 * cap), (16384, 0, 1), (4096, 4000, 2)):
        path, passes, launches, scratch = plan(n, i0, q)
        assert passes == -(-q // cap) and path in (1, 2)
        want = 0
        for j in range(passes):
            nj = n - j * cap
            p0 = min(i0, nj - 1) // 256
            want += (1 if p0 > 0 else 0) + 2 * (-(-nj // 256) - p0) - 1
        assert launches == want, (n, i0, q, launches, want)
    assert plan(600, 70, 1)[2] == plan(600, 70, cap)[2]  # the launches do not depend on the vectors in a pass
    # the scratch is monotone in n
    sc = [plan(n, 0, 1)[3] for n in range(2, 20000, 37)]
    assert all(b >= a for a, b in zip(sc, sc[1:]))
    # bad arguments
    fn = lib.fn("debug_remove_plan")
    out = (ctypes.c_int64 * 4)()
    for a in ((0, 0, 0, 0), (100, 0, -1, 0), (100, 0, 100, 0), (100, 0, 101, 0), (100, -1, 1, 0), (100, 100, 1, 0), (100, 95, 6, 0),
              (100, 10, 5, 1)):
        assert fn(*a, out) in (-1,), a
    assert fn(100, 0, 1, 0, None) == -1
    with pytest.raises(_capi.EngineError):
        plan(100, 0, 100)


def build_driver(asan=False):
    """tests/cpp/test_remove_samples with the flags of tests/cpp/Makefile (as tests.test_add_samples_host.build_driver)"""
    exe = DRIVER.with_name(DRIVER.name + ("_asan" if asan else ""))
    src = DRIVER.with_suffix(".cpp")
    deps = [src, _capi.ENGINE_SO] + list((ROOT / "include").rglob("*.h*"))
    if exe.exists() and all(exe.stat().st_mtime >= d.stat().st_mtime for d in deps):
        return exe
    cxx = os.environ.get("CXX", "g++")
    opt = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g", "-O1"] if asan else ["-O2"]
    subprocess.check_call([cxx, "-std=c++17"] + opt + ["-Wall", "-Wno-unused-variable", "-I" + str(ROOT / "include" / "limbo_amd"),
                           "-I" + str(ROOT / "oracle" / "ref_build" / "shim"), "-o", str(exe), str(src), "-L" + str(ROOT / "limbo_amd"),
                           "-lgpengine", "-Wl,-rpath,$ORIGIN/../../limbo_amd", "-Wl,-rpath,/opt/rocm/lib", "-lpthread"])
    return exe


def parse_output(stdout):
    """{case: {n, L, alpha, mu, sigma}} of the driver's `case=<name> n=.. L=.. alpha=.. mu=.. sigma=..` lines"""
    out = {}
    for ln in stdout.splitlines():
        w = dict(t.split("=", 1) for t in ln.split() if "=" in t)
        if "case" in w:
            out[w["case"]] = {k: (int(v) if k == "n" else float(v)) for k, v in w.items() if k != "case"}
    return out


HOST_CASES = ["host-first", "host-last", "host-3-64-65", "host-40-scattered", "host-everything-prior", "host-everything-refill", "host-multi",
              "host-window"]


def _check_host_output(stdout):
    out = parse_output(stdout)
    assert sorted(out) == sorted(HOST_CASES), stdout[-2000:]
    want_n = {"host-first": 119, "host-last": 119, "host-3-64-65": 117, "host-40-scattered": 80, "host-everything-prior": 0,
              "host-everything-refill": 2, "host-multi": 55, "host-window": 50}
    for name, c in out.items():
        print(name, c)
        assert c["n"] == want_n[name], (name, c)
        assert c["L"] <= 1e-12 and c["alpha"] <= 1e-9 and c["mu"] <= 1e-10 and c["sigma"] <= 1e-10, (name, c)


def test_dropin_remove_samples_host_path():
    """In host mode GP::remove_samples against a fresh compute() on the remaining samples (L 1e-12, alpha 1e-9, mu / sigma^2
    1e-10): n = 120 with R = {0}, {119}, {3, 64, 65} and 40 scattered indices; removing everything (the prior, then samples
    again); MultiGP; add_sample_windowed over 30 steps with window 50."""
    r = subprocess.run([str(build_driver())], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    _check_host_output(r.stdout)


def test_dropin_remove_samples_host_path_under_asan_ubsan():
    """The same driver as a stand-alone program with -fsanitize=address,undefined (a host build; the host path needs no GPU)
    finishes without a report."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(build_driver(asan=True))], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    _check_host_output(r.stdout)
