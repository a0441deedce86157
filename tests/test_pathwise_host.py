"""Pathwise posterior draws (include/gpe_pathwise.h) without a GPU: the reference that checks the device (tests/pathwise_ref.py)
against itself, against the posterior it must reproduce, against central differences and against the statistics a posterior draw
has; the spectral law of every kernel kind; the ABI; and the host route of the C++ drop-in — model::GP::sample_paths, PathSet and
limbo_amd::thompson_paths_batch on a host-resident model (tests/cpp/test_pathwise_host, compiled here with the flags of
tests/cpp/Makefile)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from limbo_amd import _capi
from oracle import np_oracle as O
from tests import pathwise_ref as PR
from tests import query_grad_ref as Q
from tests import test_query_grad_host as H  # run_driver and the compiler flags of the drop-in drivers

ROOT = Path(__file__).resolve().parent.parent
CPP = ROOT / "tests" / "cpp"
NOISE = Q.NOISE
MEAN_CONSTANT = 1.0  # mean::Constant of the drivers' Params

KINDS = {"se_ard": (O.SE_ARD, 3, 0), "se_ard_lambda2": (O.SE_ARD, 5, 2), "matern52": (O.MATERN52, 3, 0), "matern32": (O.MATERN32, 3, 0),
         "exp": (O.EXP, 3, 0)}


def small_case(kind, D, lam, N=90, P=2, R=200, S=3, T=9, seed=21):
    X, om = Q.make_problem(N, D, P, seed)
    th = Q.theta_of(kind, D, lam, seed)
    Om, ph, W, E = PR.make_draws(kind, th, N, D, P, R, S, seed + 1)
    return X, om, th, Om, ph, W, E, Q.make_points(X, T, seed + 2)


@pytest.mark.parametrize("shape", PR.GPU_SHAPES, ids=lambda s: "k%d_n%d_d%d_p%d_l%d" % s)
def test_reference_routes_agree(shape):
    """Cholesky against LU with extended-precision refinement at every model of tests/test_gpu_pathwise.py (at N = 4096 the draws of
    the GPU test, R = 2048 and S = 16, on sixteen points: the extended-precision residual is the cost)"""
    big = shape[1] >= 4096
    d = PR.routes_disagreement(*shape, R=2048 if big else 1000, S=16 if big else 8, T=16 if big else 70)
    print(shape, ["%.2e" % x for x in d])
    assert max(d[:2]) <= 1e-11


@pytest.mark.parametrize("R_,S", [(1, 1), (63, 3), (64, 9), (65, 65), (1, 65), (1000, 1)])
def test_reference_routes_agree_on_the_tile_edges(R_, S):
    d = PR.routes_disagreement(O.SE_ARD, 300, 3, 1, 0, R=R_, S=S)
    assert max(d[:2]) <= 1e-11


@pytest.mark.parametrize("name", list(KINDS))
def test_zero_draws_give_the_posterior_mean(name):
    """W = 0, E = 0: U = alpha, so F is k^T alpha and dF its gradient (tests/query_grad_ref.py) — the signs and the role of U"""
    kind, D, lam = KINDS[name]
    X, om, th, Om, ph, W, E, V = small_case(kind, D, lam)
    F, dF = PR.reference(kind, X, om, th, NOISE, Om, ph, np.zeros_like(W), np.zeros_like(E), V)
    kta, _, dkta, _ = Q.reference(kind, X, om, th, NOISE, V)
    for s in range(W.shape[1]):
        assert np.max(np.abs(F[:, s, :] - kta)) <= 1e-12 and np.max(np.abs(dF[:, :, s, :] - dkta)) <= 1e-12
    F0, _ = PR.reference(kind, X, om, th, NOISE, Om, ph, np.zeros_like(W), None, V, mean_q=np.full((V.shape[0], 2), 0.25))
    assert np.max(np.abs(F0 - F - 0.25)) <= 1e-14, "E = None is E = 0; mean_q is added"


@pytest.mark.parametrize("name", list(KINDS))
def test_reference_against_central_differences(name):
    kind, D, lam = KINDS[name]
    X, om, th, Om, ph, W, E, V = small_case(kind, D, lam)
    V = V[4:]  # (the Matern kernels' second derivative jumps AT a sample: differences are not a check there)
    U = PR.solve_U(kind, X, om, th, NOISE, Om, ph, W, E)
    _, dF = PR.evaluate(kind, X, th, Om, ph, W, U, V)
    h, fd = 1e-5, np.zeros_like(dF)
    for d in range(D):
        e = np.zeros(D)
        e[d] = h
        fd[:, d] = (PR.evaluate(kind, X, th, Om, ph, W, U, V + e)[0] - PR.evaluate(kind, X, th, Om, ph, W, U, V - e)[0]) / (2 * h)
    err = np.max(np.abs(fd - dF))
    print(f"{name}: {err:.2e} of {np.max(np.abs(dF)):.2e}")
    assert err <= 1e-6 * max(1.0, np.max(np.abs(dF)))


@pytest.mark.parametrize("name", list(KINDS))
def test_spectral_law(name):
    """Phi Phi^T against k(X, X) with R = 16384 features on 200 points: <= 0.06, about 8 / sqrt(R) and twice the largest measured
    (0.010 Exp .. 0.031 SE-ARD); a wrong degree of freedom or scaling misses by far more.  Seeds are fixed: a condition, not a lottery."""
    kind, D, lam = KINDS[name]
    X, _ = Q.make_problem(200, D, 1, 31)
    th = Q.theta_of(kind, D, lam, 31)
    Om, ph = PR.spectral_draws(kind, 16384, PR.freq_dim(kind, th, D), 32)
    assert Om.shape == (16384, D + lam) and ph.min() >= 0.0 and ph.max() < 2 * np.pi
    Phi = PR.features(kind, th, D, Om, ph, X)[0]
    K = O.kernel_matrix(kind, X, th, 0.0) - 1e-8 * np.eye(200)
    err = np.max(np.abs(Phi @ Phi.T - K))
    print(f"{name}: {err:.4f}")
    assert err <= 0.06


def test_statistics_of_the_reference():
    """S = 4096 draws at 16 points: their mean is the posterior mean to four standard errors, their variance the posterior variance
    to 15 % (SE-ARD, N = 200, D = 3, R = 4096; measured: 1.64 standard errors, ratios 0.93 .. 1.04)"""
    kind, N, D, S = O.SE_ARD, 200, 3, 4096
    X, om = Q.make_problem(N, D, 1, 41)
    th = Q.theta_of(kind, D, 0, 41)
    V = np.random.default_rng(42).random((16, D))
    Om, ph, W, E = PR.make_draws(kind, th, N, D, 1, 4096, S, 43)
    F, _ = PR.reference(kind, X, om, th, NOISE, Om, ph, W, E, V)
    kta, var, _, _ = Q.reference(kind, X, om, th, NOISE, V)
    zs = np.abs(F[:, :, 0].mean(axis=1) - kta[:, 0]) / np.sqrt(var / S)
    ratio = F[:, :, 0].var(axis=1, ddof=1) / var
    print(f"mean: {zs.max():.2f} standard errors; variance ratios {ratio.min():.3f} .. {ratio.max():.3f}; var {var.min():.1e} .. {var.max():.1e}")
    assert zs.max() <= 4.0
    assert ratio.min() >= 0.85 and ratio.max() <= 1.15


def test_library_exports_and_binding():
    assert _capi.ENGINE_SO.exists()
    hdr = (ROOT / "include" / "gpe_pathwise.h").read_text()
    names = re.findall(r"^int (gpe_paths_\w+)\(", hdr, flags=re.M)
    assert sorted(names) == ["gpe_paths_argmax", "gpe_paths_create", "gpe_paths_destroy", "gpe_paths_eval", "gpe_paths_info", "gpe_paths_phase_ms"]
    raw = ctypes.CDLL(str(_capi.ENGINE_SO))  # the dynamic symbol table itself, not the binding's view of it
    for n in names:
        assert hasattr(raw, n), n
    lib = _capi.load_engine()
    assert len(lib.fn("paths_create").argtypes) == 8 and len(lib.fn("paths_eval").argtypes) == 6 and len(lib.fn("paths_argmax").argtypes) == 6
    assert hasattr(_capi.Handle, "paths") and all(hasattr(_capi.Paths, m) for m in ("eval", "argmax", "close", "phase_ms"))
    assert "gpe_paths_create" not in (ROOT / "include" / "gpe.h").read_text()


# ------------------------------------------------------------------------------------------------ the C++ drop-in (shared with the GPU test)
def build_driver(name):
    """tests/cpp/<name> with the flags of tests/cpp/Makefile (which this change leaves alone)"""
    import os
    import subprocess
    drv, src = CPP / name, CPP / (name + ".cpp")
    deps = [src, CPP / "pathwise_driver.hpp", ROOT / "limbo_amd" / "libgpengine.so", ROOT / "include" / "gpe_pathwise.h"]
    deps += [ROOT / "include" / "limbo_amd" / "limbo" / p for p in ("model/gp.hpp", "model/gp/pathwise.hpp", "model/gp/query_grad.hpp",
                                                                  "acqui/thompson.hpp", "opt/batched_rprop.hpp", "opt/batch_grad_search.hpp")]
    if drv.exists() and all(drv.stat().st_mtime >= d.stat().st_mtime for d in deps):
        return drv
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-Wall", "-Wno-unused-variable", f"-I{ROOT}/include/limbo_amd",
           f"-I{ROOT}/oracle/ref_build/shim", "-o", str(drv), str(src), f"-L{ROOT}/limbo_amd", "-lgpengine",
           "-Wl,-rpath,$ORIGIN/../../limbo_amd", "-Wl,-rpath,/opt/rocm/lib", "-lpthread"]
    subprocess.check_call(cmd)
    return drv


def _row(a):
    return " ".join(repr(float(v)) for v in np.asarray(a).ravel())


def paths_case(kind, n, D, P, T, R_, S, seed, lam=0):
    X, om = Q.make_problem(n, D, P, seed)
    th = Q.theta_of(kind, D, lam, seed)
    Om, ph, W, E = PR.make_draws(kind, th, n, D, P, R_, S, seed + 1)
    return dict(kind=kind, th=th, X=X, Y=om + MEAN_CONSTANT, V=Q.make_points(X, T, seed + 2), Om=Om, ph=ph, W=W, E=E, S=S, seed=seed)


def paths_case_text(c):
    X, Y, V, W, E = c["X"], c["Y"], c["V"], c["W"], c["E"]
    R_, S, P = W.shape
    rows = [f"{c['kind']} {P} {X.shape[1]} {X.shape[0]} {V.shape[0]} {c['th'].size} {R_} {S} {c['seed']}", _row(c["th"])]
    rows += [_row(list(X[i]) + list(Y[i])) for i in range(X.shape[0])]
    rows += [_row(q) for q in V]
    # Omega0 row-major; W and E with their first index fastest (include/gpe_pathwise.h)
    rows += [_row(c["Om"]), _row(c["ph"]), _row(W.reshape(-1, order="F")), _row(E.reshape(-1, order="F"))]
    return "\n".join(rows) + "\n"


def check_paths(out, c, bar=1e-10):
    """the driver's output against numpy: <= bar max(1, max|ref|)"""
    kind, th, X, V, W = c["kind"], c["th"], c["X"], c["V"], c["W"]
    R_, S, P = W.shape
    T, D = V.shape
    mq = np.full((T, P), MEAN_CONSTANT)
    F, dF = PR.reference(kind, X, c["Y"] - MEAN_CONSTANT, th, NOISE, c["Om"], c["ph"], W, c["E"], V, mean_q=mq)
    prior, _ = PR.evaluate(kind, X[:0], th, c["Om"], c["ph"], W, None, V, mean_q=mq)
    got = dict(F=out["F"].reshape(T, S, P, order="F"), dF=out["dF"].reshape(T, D, S, P, order="F"),
               prior_F=out["prior_F"].reshape(T, S, P, order="F"))
    for k, r in (("F", F), ("dF", dF), ("prior_F", prior)):
        err = np.max(np.abs(got[k] - r)) / max(1.0, np.max(np.abs(r)))
        print(f"{k}: {err:.3e}")
        assert err <= bar, (k, err)
    assert out["eval_same"][0] == 1, "eval() is eval_grad()'s F"
    am, fm = out["argmax"].reshape(S, P, order="F").astype(int), out["fmax"].reshape(S, P, order="F")
    assert np.array_equal(am, np.argmax(got["F"], axis=0)) and np.array_equal(fm, np.max(got["F"], axis=0))
    assert out["seeded_same"][0] == 1 and out["spectral_repro"][0] == 1
    Dw = PR.freq_dim(kind, th, D)
    so, sp = out["spec_omega"].reshape(R_, Dw), out["spec_phase"]
    assert sp.shape == (R_,) and sp.min() >= 0.0 and sp.max() < 2 * np.pi and np.all(np.isfinite(so))


def thompson_case_text(n, D=3, q=4, seed=5):
    X = np.random.default_rng(seed).random((n, D))
    y = -np.sum((X - 0.3) ** 2, axis=1) + 0.5 * np.sin(7.0 * X[:, 0])
    rows = [f"{D} {n} {q} {seed}"] + [_row(list(X[i]) + [y[i]]) for i in range(n)]
    return "\n".join(rows) + "\n"


def check_thompson(out, D=3, q=4):
    prop = out["proposals"].reshape(q, D)
    print("proposals", prop, "values", out["prop_value"], "best candidates", out["cand_best"])
    assert prop.min() >= 0.0 and prop.max() <= 1.0
    assert np.all(out["prop_value"] >= out["cand_best"]), "never worse on its own path than that path's best candidate"
    assert not all(np.array_equal(prop[0], p) for p in prop[1:]), "proposals of different paths are not all equal"


@pytest.mark.parametrize("name", ["se_ard", "matern52", "matern32", "exp"])
def test_cpp_host_route(tmp_path, name):
    """a host-resident GP (n = 120): sample_paths / eval / eval_grad / argmax, the prior's paths and the seeded overload (the drivers'
    SE-ARD kernel has no Lambda: Params::kernel_squared_exp_ard::k = 0)"""
    kind, D, lam = KINDS[name]
    drv = build_driver("test_pathwise_host")
    c = paths_case(kind, 120, D, 2 if kind == O.SE_ARD else 1, 20, 96, 3, 60 + kind, lam)
    out = H.run_driver(drv, "paths", paths_case_text(c), tmp_path)
    assert out["host_resident"][0] == 1 and out["on_device"][0] == 0
    check_paths(out, c)


def test_cpp_host_thompson(tmp_path):
    drv = build_driver("test_pathwise_host")
    out = H.run_driver(drv, "thompson", thompson_case_text(120), tmp_path)
    assert out["host_resident"][0] == 1
    check_thompson(out)
