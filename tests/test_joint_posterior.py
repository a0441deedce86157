"""The joint posterior over a point batch (include/gpe_joint.h) — what can be held WITHOUT a device:

* the C-ABI: a header of its own (include/gpe.h declares none of it: every gpe_* of gpe.h has a twin in the CPU oracle, and the
  oracle has no joint posterior), exported by libgpengine.so, bound by limbo_amd._capi;
* the launch plan of the covariance product Zt Zt^T (limbo_amd/csrc/joint.hip: k = N is long and the lower 128 x 128 tiles are
  few, so every tile's k range is split over workgroups) EXECUTED IN NUMPY, as tests/test_inv_plan.py does for K^-1:
  gpe_debug_cov_plan hands out (tile i, tile j, k0, k1, partial slot) per workgroup; each is carried out literally, a tile's
  partials are added in ascending slot, and tril(Zt Zt^T) must come out;
* the host path of the C++ drop-in (model::GP::query_joint / sample below Params::gpu::min_n_for_gpu, and the empty model):
  tests/cpp/test_joint_dropin, compiled here with the flags of tests/cpp/Makefile, against numpy on the CPU oracle's factor and
  alpha."""
import ctypes
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import scipy.linalg as sla

from limbo_amd import _capi
from oracle import np_oracle as O

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("gpe_joint_query", "gpe_joint_draws", "gpe_joint_max_points", "gpe_debug_cov_plan")
TILE, KSTEP = 128, 16


def test_abi_lives_in_its_own_header(engine_lib):
    hj = (ROOT / "include" / "gpe_joint.h").read_text()
    h = (ROOT / "include" / "gpe.h").read_text()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hj), n + " is not declared in include/gpe_joint.h"
        assert not re.search(r"\b" + n + r"\s*\(", h), n + " must not be declared in include/gpe.h"
        assert hasattr(engine_lib.cdll, n), n + " is not exported by libgpengine.so"
        assert engine_lib.fn(n[4:]).argtypes is not None, n + " is not bound by _capi"
    assert '#include "gpe.h"' in hj
    for m in ("joint_query", "joint_draws", "joint_max_points"):
        assert callable(getattr(_capi.Handle, m))


# ------------------------------------------------------------------------------------------------ the plan, in numpy
_REF = {}


def _zt_and_ref(M, N):
    if (M, N) not in _REF:
        _REF.clear()  # (one shape at a time: the largest Zt is 512 MiB)
        rng = np.random.default_rng(M * 100003 + N)
        Zt = np.asfortranarray(rng.standard_normal((M, N)) / np.sqrt(N))
        _REF[(M, N)] = (Zt, np.tril(Zt @ Zt.T))
    return _REF[(M, N)]


@pytest.mark.parametrize("N", [300, 1700, 4096, 16384])
@pytest.mark.parametrize("M", [65, 128, 700, 1024, 2048, 4096])
def test_cov_plan_executed_in_numpy(engine_lib, M, N):
    Zt, ref = _zt_and_ref(M, N)
    nt = (M + TILE - 1) // TILE
    tiles = nt * (nt + 1) // 2
    for cus in (64, 256):
        plan = _capi.debug_cov_plan(engine_lib, M, N, cus)
        nslots = int(plan[:, 4].max()) + 1
        part = {}
        cover = {}
        for ti, tj, k0, k1, slot in plan.tolist():
            assert 0 <= tj <= ti < nt, "a workgroup outside the lower triangle of tiles"
            assert 0 <= k0 < k1 <= N
            assert k0 % KSTEP == 0 and (k1 % KSTEP == 0 or k1 == N), "chunk bounds are multiples of the k step except the last"
            assert (ti, tj, slot) not in part, "two workgroups for one partial tile"
            a = Zt[ti * TILE:(ti + 1) * TILE, k0:k1]
            b = Zt[tj * TILE:(tj + 1) * TILE, k0:k1]
            part[(ti, tj, slot)] = a @ b.T
            cover.setdefault((ti, tj), []).append((slot, k0, k1))
        assert len(cover) == tiles, "every lower tile has workgroups"
        got = np.zeros((M, M))
        for (ti, tj), ch in cover.items():
            ch.sort()  # ascending slot: the order of the reduction ...
            assert [c[0] for c in ch] == list(range(len(ch)))
            assert ch[0][1] == 0 and ch[-1][2] == N, "the k range of a tile starts at 0 and ends at N"
            for (s0, a0, a1), (s1, b0, b1) in zip(ch, ch[1:]):
                assert a1 == b0 and a0 < b0, "... is ascending k0, every k covered exactly once"
            acc = part[(ti, tj, 0)].copy()
            for s in range(1, len(ch)):
                acc += part[(ti, tj, s)]
            got[ti * TILE:(ti + 1) * TILE, tj * TILE:(tj + 1) * TILE] = acc
        got = np.tril(got)
        assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(np.abs(ref))
        # the point of the split: the launch fills the chip where the shape allows it (no chunk is shorter than 256 of depth)
        allowed = tiles * max(1, ((N + KSTEP - 1) // KSTEP * KSTEP) // 256)
        assert len(plan) >= min(cus, allowed), (len(plan), cus, allowed)
        assert len(plan) == tiles * nslots


def test_cov_plan_rejects_bad_arguments(engine_lib):
    f = engine_lib.fn("debug_cov_plan")
    assert f(0, 100, 256, None, 0) == -1 and f(10, 0, 256, None, 0) == -1 and f(10, 10, 0, None, 0) == -1


# ------------------------------------------------------------------------------------------------ the drop-in's host path
DRIVER = ROOT / "tests" / "cpp" / "test_joint_dropin"


def build_driver():
    """tests/cpp/test_joint_dropin with the flags of tests/cpp/Makefile (that file is not this test's to change)"""
    src = DRIVER.with_suffix(".cpp")
    deps = [src, _capi.ENGINE_SO] + list((ROOT / "include").rglob("*.h*"))
    if DRIVER.exists() and all(DRIVER.stat().st_mtime >= d.stat().st_mtime for d in deps):
        return DRIVER
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Wno-unused-variable", "-I" + str(ROOT / "include" / "limbo_amd"),
                           "-I" + str(ROOT / "oracle" / "ref_build" / "shim"), "-o", str(DRIVER), str(src), "-L" + str(ROOT / "limbo_amd"),
                           "-lgpengine", "-Wl,-rpath,$ORIGIN/../../limbo_amd", "-Wl,-rpath,/opt/rocm/lib", "-lpthread"])
    return DRIVER


def run_driver(tmp_path, kind, mean, X, Y, Q, Z, q, jitter, seed, env=None, brief=False):
    exe = build_driver()
    n, D = X.shape
    P = Y.shape[1]
    M, S = Z.shape[0], Z.shape[1]
    f = tmp_path / "in.txt"
    with open(f, "w") as fh:
        fh.write(f"{kind} {mean} {P} {D} {n} {M} {S} {q} {jitter!r} {seed}\n")
        for i in range(n):
            fh.write(" ".join(repr(float(v)) for v in list(X[i]) + list(Y[i])) + "\n")
        for v in Q:
            fh.write(" ".join(repr(float(x)) for x in v) + "\n")
        fh.write(" ".join(repr(float(x)) for x in Z.reshape(-1, order="F")) + "\n")
    r = subprocess.run([str(exe), str(f)] + (["brief"] if brief else []), capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        out[w[0]] = np.array([float(v) for v in w[1:]])
    if brief:
        return out
    out["mu"] = out["mu"].reshape(M, P, order="F")
    out["cov"] = out["cov"].reshape(M, M, order="F")
    out["F"] = out["F"].reshape(M, S, P, order="F")
    return out


def reference(oracle_lib, kind, mean, X, Y, Q, Z, jitter, noise=0.01):
    """mu, Sigma + jitter I and the draws from the CPU oracle's factor and alpha, the kernel from oracle/np_oracle.py"""
    n, D = X.shape
    P = Y.shape[1]
    M = len(Q)
    th = np.zeros(D + 1) if kind == 0 else np.zeros(2)  # the functors' default hyper-parameters
    mval = (Y.mean(axis=0) if n else np.zeros(P)) if mean == 0 else np.ones(P)  # mean::Data / mean::Constant (constant 1)
    Sig = O.kernel_cross(kind, Q, Q, th) + jitter * np.eye(M)
    kta = np.zeros((M, P))
    if n:
        h = _capi.Handle(oracle_lib)
        h.set_data(X, Y - mval)
        h.set_kernel(kind, th, noise)
        assert h.compute() == 0
        L, al = h.get_L(), h.get_alpha()
        h.close()
        Ks = O.kernel_cross(kind, X, Q, th)
        Zs = sla.solve_triangular(L, Ks, lower=True)
        Sig = Sig - Zs.T @ Zs
        kta = Ks.T @ al
    mu = kta + mval
    C = np.linalg.cholesky(Sig)
    F = mu[:, None, :] + np.einsum("mj,jsp->msp", C, Z)
    return mu, Sig, F


HOST_CASES = [(kind, mean, P, n) for kind in (0, 1) for mean in (0, 2) for P in (1, 2) for n in (0, 1, 2, 40, 200)]


@pytest.mark.parametrize("kind,mean,P,n", HOST_CASES)
def test_dropin_host_path(tmp_path, oracle_lib, kind, mean, P, n):
    D = 3 if kind == 0 else 2
    rng = np.random.default_rng(1000 * kind + 100 * mean + 10 * P + n)
    X = rng.uniform(0, 1, size=(n, D))
    Y = np.stack([np.cos((p + 1.5) * X.sum(axis=1)) + 0.3 * X[:, 0] for p in range(P)], axis=1).reshape(n, P) + 0.05 * rng.normal(size=(n, P))
    M, S, q, jitter, noise = 12, 5, 4, 1e-6, 0.01
    Q = rng.uniform(0, 1, size=(M, D))
    Z = rng.standard_normal((M, S, P))
    got = run_driver(tmp_path, kind, mean, X, Y, Q, Z, q, jitter, 7, env={"LIMBO_AMD_MIN_N_FOR_GPU": str(1 << 20)})
    mu, Sig, F = reference(oracle_lib, kind, mean, X, Y, Q, Z, jitter)
    assert n == 0 or got["host_resident"][0] == 1
    assert np.max(np.abs(got["mu"] - mu)) <= 1e-10
    assert np.max(np.abs(got["cov"] - Sig)) <= 1e-10
    assert np.array_equal(got["cov"], got["cov"].T)
    assert np.max(np.abs(got["F"] - F)) <= 1e-10
    # cov(m, m) is sigma(points[m]) without the noise (and without the clamp of gp.hpp:621-623, where that acts)
    var = got["sigma"] - noise
    live = var > np.finfo(float).eps
    assert live.any()
    assert np.max(np.abs((np.diag(got["cov"]) - jitter - var)[live])) <= 1e-12
    assert list(got["seed_repeat"]) == [1, 1], "the same seed gives the same draws, another seed other ones"
    assert len(got["thompson"]) == q and np.array_equal(got["thompson"], got["thompson_host"])
