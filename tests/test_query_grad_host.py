"""The posterior's gradient in the query point (include/gpe_query_grad.h) without a GPU: the reference that checks the device
(tests/query_grad_ref.py) against central differences and against itself, the ABI (a header of its own, exported by libgpengine.so,
bound by limbo_amd._capi), and the host route of the C++ drop-in — model::GP::query_grad_batch, acqui::UCB / EI::batch_grad and
opt::BatchGradSearch on a host-resident model (tests/cpp/test_query_grad_host, compiled here with the flags of tests/cpp/Makefile)."""
import ctypes
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest
from scipy.special import erfc

from limbo_amd import _capi
from oracle import np_oracle as O
from tests import query_grad_ref as R

ROOT = Path(__file__).resolve().parent.parent
CPP = ROOT / "tests" / "cpp"
NOISE = R.NOISE
MEAN_CONSTANT = 1.0  # mean::Constant of the drivers' Params
UCB_ALPHA = 0.5      # defaults::acqui_ucb::alpha

KINDS = {"se_ard": (O.SE_ARD, 0), "se_ard_lambda2": (O.SE_ARD, 2), "matern52": (O.MATERN52, 0), "matern32": (O.MATERN32, 0),
         "exp": (O.EXP, 0)}


@pytest.mark.parametrize("name", list(KINDS))
def test_reference_against_central_differences(name):
    """d/dv of np_oracle's own mu and sigma^2 (oracle/np_oracle.query, another restatement of gp.hpp:613-632) by central
    differences of step 1e-5: <= 1e-6 relative to the largest component (the differences themselves are good to ~1e-7 h^2-wise)"""
    kind, lam = KINDS[name]
    N, D, P, M, h = 90, 3, 2, 7, 1e-5
    X, om = R.make_problem(N, D, P, 21)
    th = R.theta_of(kind, D, lam, 21)
    V = R.make_points(X, M, 22)[4:]  # (the Matern kernels' second derivative jumps AT a sample: differences are not a check there)
    _, L, alpha = O.gp_fit(kind, X, om, th, NOISE)
    kta, var, dkta, dvar = R.reference(kind, X, om, th, NOISE, V)
    k0, v0 = O.query(kind, X, th, L, alpha, V)
    assert np.max(np.abs(kta - k0)) <= 1e-10 and np.max(np.abs(var - v0)) <= 1e-10
    fd_k, fd_v = np.zeros_like(dkta), np.zeros_like(dvar)
    for d in range(D):
        e = np.zeros(D)
        e[d] = h
        kp, vp = O.query(kind, X, th, L, alpha, V + e)
        km, vm = O.query(kind, X, th, L, alpha, V - e)
        fd_k[:, d, :] = (kp - km) / (2 * h)
        fd_v[:, d] = (vp - vm) / (2 * h)
    ek = np.max(np.abs(fd_k - dkta)) / np.max(np.abs(dkta))
    ev = np.max(np.abs(fd_v - dvar)) / np.max(np.abs(dvar))
    print(f"{name}: dkta {ek:.2e} dvar {ev:.2e}")
    assert ek <= 1e-6 and ev <= 1e-6


@pytest.mark.parametrize("shape", R.GPU_SHAPES, ids=lambda s: "k%d_n%d_d%d_p%d_l%d" % s)
def test_reference_routes_agree(shape):
    """Cholesky solves against LU with extended-precision refinement at every shape of tests/test_gpu_query_grad.py (sixteen
    points at N = 4096, where the extended-precision residual of more is minutes of host work)"""
    d = R.routes_disagreement(*shape, M=16 if shape[1] >= 4096 else 64)
    print(shape, ["%.2e" % x for x in d])
    assert max(d) <= 1e-10


def test_library_exports_and_binding():
    assert _capi.ENGINE_SO.exists()
    raw = ctypes.CDLL(str(_capi.ENGINE_SO))  # the dynamic symbol table itself, not the binding's view of it
    assert hasattr(raw, "gpe_query_batch_grad") and hasattr(raw, "gpe_query_grad_phase_ms")
    lib = _capi.load_engine()
    assert len(lib.fn("query_batch_grad").argtypes) == 7 and len(lib.fn("query_grad_phase_ms").argtypes) == 2
    assert hasattr(_capi.Handle, "query_batch_grad") and hasattr(_capi.Handle, "query_grad_phase_ms")
    hdr = (ROOT / "include" / "gpe_query_grad.h").read_text()
    assert "gpe_query_batch_grad" in hdr and "gpe_query_grad_phase_ms" in hdr
    assert "gpe_query_batch_grad" not in (ROOT / "include" / "gpe.h").read_text()


# ------------------------------------------------------------------------------------------------ the C++ drop-in (shared with the GPU test)
def build_driver(name):
    """tests/cpp/<name> with the flags of tests/cpp/Makefile (which this change leaves alone)"""
    drv, src = CPP / name, CPP / (name + ".cpp")
    deps = [src, CPP / "query_grad_driver.hpp", ROOT / "limbo_amd" / "libgpengine.so", ROOT / "include" / "gpe_query_grad.h"]
    deps += [ROOT / "include" / "limbo_amd" / "limbo" / p for p in ("model/gp.hpp", "model/gp/query_grad.hpp", "acqui/ucb.hpp", "acqui/ei.hpp",
                                                                  "acqui/afun_gradient.hpp", "acqui/beliefs.hpp", "opt/batch_search.hpp", "opt/batch_grad_search.hpp")]
    if drv.exists() and all(drv.stat().st_mtime >= d.stat().st_mtime for d in deps):
        return drv
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-Wall", "-Wno-unused-variable", f"-I{ROOT}/include/limbo_amd",
           f"-I{ROOT}/oracle/ref_build/shim", "-o", str(drv), str(src), f"-L{ROOT}/limbo_amd", "-lgpengine",
           "-Wl,-rpath,$ORIGIN/../../limbo_amd", "-Wl,-rpath,/opt/rocm/lib", "-lpthread"]
    subprocess.check_call(cmd)
    return drv


def run_driver(drv, mode, text, tmp_path, env=None):
    f = tmp_path / f"{mode}.txt"
    f.write_text(text)
    r = subprocess.run([str(drv), mode, str(f)], capture_output=True, text=True, timeout=300, env={**os.environ, **(env or {})})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        out[w[0]] = np.array([float(v) for v in w[1:]])
    return out


def grad_case_text(kind, th, X, Y, V):
    rows = [f"{kind} {Y.shape[1]} {X.shape[1]} {X.shape[0]} {V.shape[0]} {th.size}", " ".join(repr(float(v)) for v in th)]
    rows += [" ".join(repr(float(v)) for v in list(X[i]) + list(Y[i])) for i in range(X.shape[0])]
    rows += [" ".join(repr(float(v)) for v in q) for q in V]
    return "\n".join(rows) + "\n"


def dropin_reference(kind, th, X, Y, V):
    """what the driver prints, from numpy: the model's four outputs (mean::Constant added, clamp, + noise) and the two acquisition
    functors with limbo_amd::FirstElem; gradients as (M, D) / (M, D, P)"""
    om = Y - MEAN_CONSTANT
    kta, var, dkta, dvar = R.reference(kind, X, om, th, NOISE, V)
    clamp = var <= np.finfo(float).eps
    s2 = np.where(clamp, 0.0, var) + NOISE
    ds2 = np.where(clamp[:, None], 0.0, dvar)
    mu = kta + MEAN_CONSTANT
    sig = np.sqrt(s2)
    ref = dict(mu=mu, s2=s2, dmu=dkta, ds2=ds2, ucb=mu[:, 0] + UCB_ALPHA * sig, ducb=dkta[:, :, 0] + UCB_ALPHA / (2 * sig)[:, None] * ds2)
    fplus = np.max(R.reference(kind, X, om, th, NOISE, X)[0][:, 0] + MEAN_CONSTANT)  # acqui/ei.hpp: the best predicted mean at the samples
    Z = (mu[:, 0] - fplus) / sig
    phi, Phi = np.exp(-0.5 * Z * Z) / np.sqrt(2 * np.pi), 0.5 * erfc(-Z / np.sqrt(2))
    ref["ei"] = (mu[:, 0] - fplus) * Phi + sig * phi
    ref["dei"] = Phi[:, None] * dkta[:, :, 0] + phi[:, None] * ds2 / (2 * sig)[:, None]
    return ref


def check_dropin(out, ref, bar=1e-8):
    M, D, P = ref["dmu"].shape
    got = dict(mu=out["mu"].reshape(P, M).T, s2=out["s2"], dmu=out["dmu"].reshape(P, D, M).transpose(2, 1, 0), ds2=out["ds2"].reshape(D, M).T,
               ucb=out["ucb"], ducb=out["ducb"].reshape(D, M).T, ei=out["ei"], dei=out["dei"].reshape(D, M).T)
    for k, g in got.items():
        err = np.max(np.abs(g - ref[k])) / max(1.0, np.max(np.abs(ref[k])))
        print(f"{k}: {err:.3e}")
        assert err <= bar, (k, err)
    one = out["one"]
    assert abs(one[0] - ref["ucb"][0]) <= bar and np.max(np.abs(one[1:1 + D] - ref["ducb"][0])) <= bar * max(1.0, np.max(np.abs(ref["ducb"])))
    assert abs(one[1 + D] - ref["ei"][0]) <= bar and np.max(np.abs(one[2 + D:] - ref["dei"][0])) <= bar * max(1.0, np.max(np.abs(ref["dei"])))
    assert out["same_bits"][0] == 1, "operator() without gradient is what it was"
    assert out["vs_query_batch"][0] <= 1e-10, "mu and sigma^2 are query_batch's"


def dropin_problem(kind, n, D, P, M, seed):
    X, om = R.make_problem(n, D, P, seed)
    return kind, R.theta_of(kind, D, 0, seed), X, om + MEAN_CONSTANT, R.make_points(X, M, seed + 1)


def search_case_text(n=200, D=4, bins=8, seed=3):
    """a GP fitted to -|x - 0.3|^2 in D = 4"""
    X = np.random.default_rng(seed).random((n, D))
    y = -np.sum((X - 0.3) ** 2, axis=1)
    rows = [f"{D} {n} {bins}"] + [" ".join(repr(float(v)) for v in list(X[i]) + [y[i]]) for i in range(n)]
    return "\n".join(rows) + "\n"


HOST_ENV = {"LIMBO_AMD_HOST_BATCH_CROSSOVER": str(10 ** 12)}  # every batch of a host-resident model stays on the host


@pytest.mark.parametrize("kind", [O.SE_ARD, O.MATERN52, O.MATERN32, O.EXP])
def test_cpp_host_route(tmp_path, kind):
    """a host-resident GP (n = 120): query_grad_batch, UCB / EI::batch_grad and operator() with a gradient against numpy: 1e-8"""
    drv = build_driver("test_query_grad_host")
    case = dropin_problem(kind, 120, 3, 2 if kind == O.SE_ARD else 1, 30, 40 + kind)
    out = run_driver(drv, "grad", grad_case_text(*case), tmp_path, HOST_ENV)
    assert out["host_resident"][0] == 1
    check_dropin(out, dropin_reference(*case))


def test_cpp_host_search(tmp_path):
    """BatchGradSearch on the posterior mean of a host-resident GP (n = 120): at least the best of the 9^4 grid, less 1e-9"""
    drv = build_driver("test_query_grad_host")
    out = run_driver(drv, "search", search_case_text(n=120), tmp_path, HOST_ENV)
    assert out["host_resident"][0] == 1
    print("grid", out["grid_best"][0], "search", out["search_value"][0], out["search_point"])
    assert out["search_value"][0] >= out["grid_best"][0] - 1e-9
