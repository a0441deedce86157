"""gpe_add_samples (include/gpe_append.h) without a GPU: the ABI (a header of its own, exported by libgpengine.so, bound by
limbo_amd._capi, gpe.h's symbol set untouched — the CPU oracle has no batched call) and the host path of the C++ drop-in's
model::GP::add_samples / MultiGP::add_samples (tests/cpp/test_add_samples, compiled here with the flags of tests/cpp/Makefile)
against the reference's own add_sample loop (oracle/_ref), to the tolerances of tests/test_host_path.py."""
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from limbo_amd import _capi
from oracle import binding as OB

ROOT = Path(__file__).resolve().parent.parent
DRIVER = ROOT / "tests" / "cpp" / "test_add_samples"
# gpe.h's declared entry points as this change found them (tests/test_abi.py holds the oracle to the C-ABI among them)
GPE_H_SYMBOLS = """gpe_add_sample gpe_batch_compute gpe_batch_hp_objective gpe_batch_log_lik gpe_clone gpe_clone_to gpe_compute
gpe_compute_inv_kernel gpe_create gpe_debug_chain_split gpe_debug_inv_plan gpe_debug_live_buffers gpe_debug_ragged_split gpe_debug_tail_order
gpe_debug_tail_plan gpe_debug_tri_tile_map gpe_destroy gpe_device_count gpe_epoch gpe_flow_retries gpe_get_K gpe_get_Kinv gpe_get_L
gpe_get_alpha gpe_get_device gpe_get_loo_weights gpe_get_phase_ms gpe_get_stream gpe_handover_reruns gpe_hbm_stream_peak
gpe_hp_objective gpe_last_error gpe_log_lik gpe_log_lik_grad gpe_log_loo_cv gpe_log_loo_cv_grad gpe_mfma_f64_peak gpe_nb_samples
gpe_query_batch gpe_query_batch_cross gpe_reset_phase_ms gpe_set_K_host gpe_set_L gpe_set_alpha gpe_set_data gpe_set_data_device
gpe_set_kernel gpe_set_obs_mean gpe_set_profiling gpe_small_calls gpe_sparsify gpe_synchronize gpe_trace gpe_trace_dump
gpe_update_alpha gpe_version gpe_xproc_waits""".split()


def _declared(header):
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / header).read_text(), flags=re.S)
    return set(re.findall(r"\b(gpe_[A-Za-z0-9_]+)\s*\(", txt))


def test_append_header_declares_the_call_and_gpe_h_is_unchanged():
    app = _declared("gpe_append.h")
    assert {"gpe_add_samples", "gpe_append_max_chunk"} <= app
    core = _declared("gpe.h")
    assert not ({"gpe_add_samples", "gpe_append_max_chunk"} & core)
    assert sorted(core) == sorted(GPE_H_SYMBOLS)


def test_library_exports_and_binding():
    assert _capi.ENGINE_SO.exists()
    import ctypes

    raw = ctypes.CDLL(str(_capi.ENGINE_SO))  # the dynamic symbol table itself, not the binding's view of it
    assert hasattr(raw, "gpe_add_samples") and hasattr(raw, "gpe_append_max_chunk")
    lib = _capi.load_engine()
    assert lib.fn("add_samples").argtypes is not None and len(lib.fn("add_samples").argtypes) == 6
    c = _capi.append_max_chunk(lib)  # host only: no device is touched
    assert 1 <= c <= 128
    assert hasattr(_capi.Handle, "add_samples")


def test_tail_scratch_covers_every_order_a_call_can_see():
    """The tail's split of the k range (gpe_debug_append_slices): the slices cover [0, n), there are at most 256 of them, and —
    the slice count is NOT monotone above 65 536 samples (65 536: 256 slices of 256 columns, 65 537: 241 of 272) — what a call
    reserves for its final order holds the partial matrices and S of EVERY order below it, so a batch whose chunks straddle
    such a drop (n0 = 65 500, q = 64) never writes past its scratch."""
    lib = _capi.load_engine()
    ch = _capi.append_max_chunk(lib)
    ns = sorted(set(list(range(0, 1500)) + list(range(61000, 70500)) + list(range(65536 - 300, 200000, 997))
                    + [4096 * k + d for k in range(15, 70) for d in (-1, 0, 1, 2, 127, 128, 129)]))
    info = {n: _capi.debug_append_slices(lib, n) for n in ns}
    assert info[65536][:2] == (256, 256) and info[65537][1] < 256  # the drop this test is about
    worst = 0  # the largest slice count of any order seen so far (ascending n)
    for n in ns:
        ks, nsl, cap, doubles = info[n]
        assert 1 <= nsl <= 256 and ks % 16 == 0 and ks * nsl >= n and ks * (nsl - 1) < max(n, 1)
        worst = max(worst, nsl)
        assert cap >= worst, (n, cap, worst)
        assert doubles == (cap + 1) * ch * ch
    for n0, q in ((65500, 64), (65000, 1024), (69600, 130), (61900, 100)):  # every order a chunk of such a call starts from
        cap = _capi.debug_append_slices(lib, n0 + q)[2]
        assert all(_capi.debug_append_slices(lib, n)[1] <= cap for n in range(n0, n0 + q + 1))
    assert lib.fn("debug_append_slices")(-1, None, None, None, None) == -1


def build_driver(asan=False):
    """tests/cpp/test_add_samples with the flags of tests/cpp/Makefile (that file is not this test's to change)"""
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


def write_input(path, kind, mean, X, Y, n0, Q):
    n1, D = X.shape
    with open(path, "w") as fh:
        fh.write(f"{kind} {mean} {Y.shape[1]} {D} {n0} {n1} {len(Q)}\n")
        for i in range(n1):
            fh.write(" ".join(repr(float(v)) for v in list(X[i]) + list(Y[i])) + "\n")
        for q in Q:
            fh.write(" ".join(repr(float(v)) for v in q) + "\n")


def parse_output(stdout):
    out, cur = {}, None
    for ln in stdout.splitlines():
        w = ln.split()
        if not w:
            continue
        if w[0] in ("batch", "loop"):
            cur = out.setdefault(w[0], {"n": int(w[2])})
        elif w[0].startswith("multi_"):
            out[w[0]] = np.array([float(v) for v in w[1:]])
        else:
            cur[w[0]] = np.array([float(v) for v in w[1:]])
    return out


def problem(kind, mean, P, D, n1):
    rng = np.random.default_rng(100 * kind + 10 * mean + P + n1)
    X = rng.uniform(-1, 1, size=(n1, D))
    Y = np.stack([np.cos((p + 1.5) * X.sum(axis=1)) + 0.3 * X[:, 0] for p in range(P)], axis=1) + 0.05 * rng.normal(size=(n1, P))
    Q = np.concatenate([rng.uniform(-1, 1, size=(4, D)), X[:1], X[-1:]])  # two AT training points, one of them a new sample
    return X, Y, Q


CASES = [(0, 0, 1, 3, 12, 30), (0, 1, 2, 2, 20, 45), (1, 0, 1, 4, 5, 40), (1, 2, 3, 2, 12, 30), (3, 0, 2, 2, 20, 45), (3, 1, 3, 3, 5, 40)]


@pytest.mark.skipif(not OB.ref_available(), reason="no oracle/_ref/libref.so")
@pytest.mark.parametrize("kind,mean,P,D,n0,n1", CASES)
def test_add_samples_host_path_vs_reference(tmp_path, kind, mean, P, D, n0, n1):
    """model::GP::add_samples below the host threshold against limbo::model::GP's own add_sample loop: L 1e-12, alpha 1e-9,
    log-lik 1e-11, mu 1e-10, sigma^2 1e-8."""
    X, Y, Q = problem(kind, mean, P, D, n1)
    f = tmp_path / "in.txt"
    write_input(f, kind, mean, X, Y, n0, Q)
    r = subprocess.run([str(build_driver()), str(f)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = parse_output(r.stdout)["batch"]
    assert got["n"] == n1 and got["status"][0] == 0
    ref = OB.RefGP(kind, D, P, mean={0: OB.MEAN_DATA, 1: OB.MEAN_NULL, 2: OB.MEAN_CONSTANT}[mean], noise=0.01, constant=1.0)
    ref.compute(X[:n0], Y[:n0])
    for i in range(n0, n1):
        ref.add_sample(X[i], Y[i])
    Lr = ref.matrixL()
    L = got["L"].reshape(n1, n1, order="F")
    assert np.all(np.triu(L, 1) == 0.0)
    assert np.max(np.abs(L - Lr)) <= 1e-12 * np.max(np.abs(Lr))
    assert np.max(np.abs(got["alpha"].reshape(n1, P, order="F") - ref.alpha())) <= 1e-9 * np.max(np.abs(ref.alpha()))
    assert abs(got["log_lik"][0] - ref.log_lik()) <= 1e-11 * abs(ref.log_lik())
    mur, s2r = ref.query(Q)
    assert np.max(np.abs(got["mu"].reshape(len(Q), P) - mur)) <= 1e-10 * max(1.0, np.max(np.abs(mur)))
    assert np.max(np.abs(got["sigma"] - s2r) / s2r) <= 1e-8
    ref.close()


@pytest.mark.parametrize("kind,mean,P,D,n0,n1", [CASES[1], CASES[5]])
def test_multi_gp_add_samples_equals_the_add_sample_loop(tmp_path, kind, mean, P, D, n0, n1):
    """MultiGP::add_samples == q MultiGP::add_sample calls: mu at four points to 1e-10."""
    X, Y, Q = problem(kind, mean, P, D, n1)
    f = tmp_path / "in.txt"
    write_input(f, kind, mean, X, Y, n0, Q[:4])
    r = subprocess.run([str(build_driver()), str(f)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = parse_output(r.stdout)
    a, b = out["multi_batch"], out["multi_loop"]
    assert a.size == 4 * P and np.all(np.isfinite(a))
    assert np.max(np.abs(a - b)) <= 1e-10 * max(1.0, np.max(np.abs(b)))


def test_add_samples_host_path_under_asan_ubsan(tmp_path):
    """The same driver with -fsanitize=address,undefined (a host build; the host path needs no GPU) finishes without a report."""
    X, Y, Q = problem(0, 0, 2, 3, 40)
    f = tmp_path / "in.txt"
    write_input(f, 0, 0, X, Y, 5, Q)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(build_driver(asan=True)), str(f)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "batch n 40" in r.stdout and "multi_loop" in r.stdout
