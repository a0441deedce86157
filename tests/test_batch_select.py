"""Greedy batch selection with hallucinated observations (include/gpe_batch_select.h) — what can be held WITHOUT a device:

* the C-ABI: a header of its own (include/gpe.h declares none of it: the CPU oracle mirrors that header and has no such call),
  exported by libgpengine.so, bound by limbo_amd._capi;
* the launch plan of one round's column product Zt z_j (limbo_amd/csrc/select.hip: the k range is split over workgroups so that
  the chip streams at any M) EXECUTED IN NUMPY, as tests/test_joint_posterior.py does for the covariance product:
  gpe_debug_select_plan hands out (m0, m1, k0, k1, partial slot) per workgroup; each is carried out literally, the partials of an
  m are added in ascending slot, and Zt @ Zt[j] must come out;
* the host path of the C++ drop-in (model::GP::select_batch, acqui/batch_select.hpp below Params::gpu::min_n_for_gpu, and the
  empty model): tests/cpp/test_batch_select_dropin, compiled here with the flags of tests/cpp/Makefile, against the recursion in
  numpy on the CPU oracle's factor and alpha.

The reference of every comparison (also of tests/test_gpu_batch_select.py) is ref_select() below: the recursion of the header on a
covariance Sig formed in numpy.  cross_check() is an independent route to its var_q (a block solve instead of the rank-1 steps)."""
import math
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import scipy.linalg as sla
from scipy.special import erfc

from limbo_amd import _capi
from oracle import np_oracle as O

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("gpe_select_batch", "gpe_select_phase_ms", "gpe_debug_select_plan")
UCB, EI, VAR = 0, 1, 2
EPS = np.finfo(float).eps
KSTEP = 16


# ------------------------------------------------------------------------------------------------ the reference
def score_fn(rule, mu, var, var_add, param):
    s2 = np.where(var <= EPS, 0.0, var) + var_add
    if rule == VAR:
        return s2
    sig = np.sqrt(s2)
    if rule == UCB:
        return mu + param * sig
    X = mu - param
    with np.errstate(divide="ignore", invalid="ignore"):
        Z = X / sig
        v = X * 0.5 * erfc(-Z / math.sqrt(2.0)) + sig * np.exp(-0.5 * Z * Z) / math.sqrt(2.0 * math.pi)
    return np.where(sig < 1e-10, 0.0, v)


def ref_select(Sig, mu, q, rule, param, var_add, lam, distinct):
    """the recursion of include/gpe_batch_select.h: dict(status, idx, score, var, W, margin) — margin[t] = (best - runner-up) / |best|
    of round t's scores (inf where one candidate is left)"""
    M = Sig.shape[0]
    var = np.diag(Sig).copy()
    W = np.zeros((M, q))
    idx, sc, margin = [], [], []
    status = 0
    for t in range(q):
        s = score_fn(rule, mu, var, var_add, param)
        if distinct and idx:
            s[np.array(idx)] = -np.inf
        j = int(np.argmax(s))  # (the first of equal values: the lowest index)
        rest = np.delete(s, j)
        rest = rest[np.isfinite(rest)]
        if rest.size == 0 or (s[j] == 0 and rest.max() < 0):
            margin.append(np.inf)
        else:
            margin.append((s[j] - rest.max()) / abs(s[j]) if s[j] != 0 else 0.0)
        idx.append(j)
        sc.append(s[j])
        c = Sig[:, j] - W[:, :t] @ W[j, :t]
        piv = c[j] + lam
        if not (piv > 0 and np.isfinite(piv)):
            status = t + 1
            break
        W[:, t] = c / math.sqrt(piv)
        var = var - W[:, t] ** 2
    return dict(status=status, idx=np.array(idx), score=np.array(sc), var=var, W=W, margin=np.array(margin))


def cross_check(Sig, ref, lam):
    """var_q = diag Sig - Sig[:, J] (Sig[J, J] + lam I)^-1 Sig[J, :]: max |difference| to the recursion's var"""
    J = ref["idx"]
    A = Sig[np.ix_(J, J)] + lam * np.eye(len(J))
    return np.max(np.abs(np.diag(Sig) - np.einsum("mj,jm->m", Sig[:, J], np.linalg.solve(A, Sig[J, :])) - ref["var"]))


def assert_clear(ref, exact_ties=False):
    """identical indices are a fair demand only where the reference's own winner is clear: a precondition on the inputs, not a
    skip.  exact_ties: a margin of exactly 0 is the header's tie rule at work (the prior: every candidate has the same variance)"""
    m = ref["margin"]
    ok = (m >= 1e-6) | ((m == 0.0) if exact_ties else False)
    assert np.all(ok), f"the reference's margin is {m.min():.3e} in round {int(m.argmin())}: change the seed of the inputs"


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_abi_lives_in_its_own_header(engine_lib):
    hs = (ROOT / "include" / "gpe_batch_select.h").read_text()
    h = (ROOT / "include" / "gpe.h").read_text()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hs), n + " is not declared in include/gpe_batch_select.h"
        assert not re.search(r"\b" + n + r"\s*\(", h), n + " must not be declared in include/gpe.h"
        assert hasattr(engine_lib.cdll, n), n + " is not exported by libgpengine.so"
        assert engine_lib.fn(n[4:]).argtypes is not None, n + " is not bound by _capi"
    assert '#include "gpe.h"' in hs
    for m in ("select_batch", "select_phase_ms"):
        assert callable(getattr(_capi.Handle, m))
    assert callable(_capi.debug_select_plan)
    assert (_capi.SELECT_UCB, _capi.SELECT_EI, _capi.SELECT_VAR) == (0, 1, 2)
    for name, val in (("GPE_SELECT_UCB", 0), ("GPE_SELECT_EI", 1), ("GPE_SELECT_VAR", 2)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(val) + r"\b", hs)


# ------------------------------------------------------------------------------------------------ the plan, in numpy
@pytest.mark.parametrize("N", [1, 40, 300, 1700, 16384])
@pytest.mark.parametrize("M", [1, 65, 129, 700, 4096])
def test_select_plan_executed_in_numpy(engine_lib, M, N):
    rng = np.random.default_rng(M * 100003 + N)
    Zt = np.asfortranarray(rng.standard_normal((M, N)) / math.sqrt(N))
    j = M // 3
    z = Zt[j].copy()
    ref = Zt @ z
    for cus in (64, 256):
        plan = _capi.debug_select_plan(engine_lib, M, N, cus)
        part = {}
        tiles = {}
        for m0, m1, k0, k1, slot in plan.tolist():
            assert 0 <= m0 < m1 <= M and 0 <= k0 < k1 <= N
            assert k0 % KSTEP == 0 and (k1 % KSTEP == 0 or k1 == N), "chunk bounds are multiples of the k step except the last"
            assert m0 % 2 == 0, "16-byte loads: a workgroup's first m is even"
            assert (m0, slot) not in part, "two workgroups for one partial"
            part[(m0, slot)] = Zt[m0:m1, k0:k1] @ z[k0:k1]
            tiles.setdefault((m0, m1), []).append((slot, k0, k1))
        edges = sorted(tiles)
        assert edges[0][0] == 0 and edges[-1][1] == M and all(a[1] == b[0] for a, b in zip(edges, edges[1:])), "every m covered exactly once"
        got = np.zeros(M)
        for (m0, m1), ch in tiles.items():
            ch.sort()  # ascending slot: the order of the reduction ...
            assert [c[0] for c in ch] == list(range(len(ch)))
            assert ch[0][1] == 0 and ch[-1][2] == N, "the k range of an m-tile starts at 0 and ends at N"
            for (s0, a0, a1), (s1, b0, b1) in zip(ch, ch[1:]):
                assert a1 == b0 and a0 < b0, "... is ascending k0, every k covered exactly once"
            acc = part[(m0, 0)].copy()
            for s in range(1, len(ch)):
                acc += part[(m0, s)]
            got[m0:m1] = acc
        assert np.max(np.abs(got - ref)) <= 1e-13 * max(1.0, np.max(np.abs(ref)))
        # the point of the split: two or more workgroups per compute unit wherever the shape allows it (no chunk under 32 of depth)
        allowed = len(tiles) * max(1, ((N + KSTEP - 1) // KSTEP) // 2)
        assert len(plan) >= min(2 * cus, allowed), (len(plan), cus, allowed)
        assert len(plan) == len(tiles) * (int(plan[:, 4].max()) + 1)


def test_select_plan_rejects_bad_arguments(engine_lib):
    f = engine_lib.fn("debug_select_plan")
    assert f(0, 100, 256, None, 0) == -1 and f(10, 0, 256, None, 0) == -1 and f(10, 10, 0, None, 0) == -1


# ------------------------------------------------------------------------------------------------ the drop-in's host path
DRIVER = ROOT / "tests" / "cpp" / "test_batch_select_dropin"
NOISE, ALPHA = 0.01, 2.0  # Params::kernel::noise, Params::acqui_ucb::alpha of the driver


def build_driver():
    """tests/cpp/test_batch_select_dropin with the flags of tests/cpp/Makefile (that file is not this test's to change)"""
    src = DRIVER.with_suffix(".cpp")
    deps = [src, _capi.ENGINE_SO] + list((ROOT / "include").rglob("*.h*"))
    if DRIVER.exists() and all(DRIVER.stat().st_mtime >= d.stat().st_mtime for d in deps):
        return DRIVER
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Wno-unused-variable", "-I" + str(ROOT / "include" / "limbo_amd"),
                           "-I" + str(ROOT / "oracle" / "ref_build" / "shim"), "-o", str(DRIVER), str(src), "-L" + str(ROOT / "limbo_amd"),
                           "-lgpengine", "-Wl,-rpath,$ORIGIN/../../limbo_amd", "-Wl,-rpath,/opt/rocm/lib", "-lpthread"])
    return DRIVER


def run_driver(tmp_path, kind, mean, X, Y, Q, q, agg, Yq=None, env=None):
    exe = build_driver()
    n, D = X.shape
    P = Y.shape[1]
    f = tmp_path / "in.txt"
    with open(f, "w") as fh:
        fh.write(f"{kind} {mean} {P} {D} {n} {len(Q)} {q} {agg} {int(Yq is not None)}\n")
        for i in range(n):
            fh.write(" ".join(repr(float(v)) for v in list(X[i]) + list(Y[i])) + "\n")
        for v in Q:
            fh.write(" ".join(repr(float(x)) for x in v) + "\n")
        if Yq is not None:
            for v in Yq:
                fh.write(" ".join(repr(float(x)) for x in v) + "\n")
    r = subprocess.run([str(exe), str(f)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        out[w[0]] = np.array([float(v) for v in w[1:]])
    return out


def dropin_problem(kind, P, n, M, seed):
    D = 3 if kind == 0 else 2
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, size=(n, D))
    Y = np.stack([np.cos((p + 1.5) * X.sum(axis=1)) + 0.3 * X[:, 0] for p in range(P)], axis=1).reshape(n, P) + 0.05 * rng.normal(size=(n, P))
    return X, Y, rng.uniform(0, 1, size=(M, D))


def dropin_reference(oracle_lib, kind, mean, X, Y, Q, agg):
    """(Sig, mu (complete: the mean functor added, the aggregator applied), f+ as acqui::EI forms it) from the CPU oracle's factor"""
    n, D = X.shape
    P = Y.shape[1]
    th = np.zeros(D + 1) if kind == 0 else np.zeros(2)  # the functors' default hyper-parameters
    mval = (Y.mean(axis=0) if n else np.zeros(P)) if mean == 0 else np.ones(P)  # mean::Data / mean::Constant (constant 1)
    Sig = O.kernel_cross(kind, Q, Q, th)
    if n == 0:
        return Sig, np.full(len(Q), mval[agg]), 0.0
    h = _capi.Handle(oracle_lib)
    h.set_data(X, Y - mval)
    h.set_kernel(kind, th, NOISE)
    assert h.compute() == 0
    L, al = h.get_L(), h.get_alpha()
    h.close()
    Ks = O.kernel_cross(kind, X, Q, th)
    Zs = sla.solve_triangular(L, Ks, lower=True)
    fplus = np.max((O.kernel_cross(kind, X, X, th).T @ al + mval)[:, agg])
    return Sig - Zs.T @ Zs, (Ks.T @ al + mval)[:, agg], fplus


def check_dropin(got, Sig, mu, fplus, q, exact_ties=False, tol=1e-8):
    """the driver's lines against the recursion on (Sig, mu): the helpers' indices, select_batch's indices and scores, and the
    first pick against the arg-max of acqui::UCB::batch / acqui::EI::batch"""
    for name, rule, param, va, lam, distinct, mm in (("ucb", UCB, ALPHA, NOISE, NOISE, True, mu), ("ei", EI, fplus, NOISE, NOISE, True, mu),
                                                       ("var", VAR, 0.0, 0.0, NOISE, False, np.zeros_like(mu))):
        ref = ref_select(Sig, mm, q, rule, param, va, lam, distinct)
        assert ref["status"] == 0
        assert_clear(ref, exact_ties)
        assert cross_check(Sig, ref, lam) <= 1e-12
        d = np.max(np.abs(got[name + "_score"] - ref["score"]))
        print(f"{name}: max|score - ref| = {d:.3e}, smallest margin {ref['margin'].min():.3e}")
        assert np.array_equal(got[name + "_idx"], ref["idx"])
        assert d <= tol
        if name == "ucb":
            assert np.array_equal(got["bucb"], ref["idx"]), "bucb_batch (the shortcut for a constant mean included) is the recursion"
        if name == "ei" and got.get("_n", 1) > 0:  # (without samples the helper does not ask the model: see the caller)
            assert np.array_equal(got["ei"], ref["idx"]), "believer_ei_batch is the recursion"
    assert got["bucb"][0] == got["ucb_argmax"][0] and got["ei"][0] == got["ei_argmax"][0], "the first pick is the acquisition's arg-max"


# (kind, mean, P, n, agg): the prior; one sample; Matern-5/2 with the Data mean; two outputs with the second-element aggregator
HOST_CASES = [(0, 0, 1, 0, 0), (0, 0, 1, 1, 0), (1, 0, 1, 40, 0), (0, 0, 2, 200, 1)]


@pytest.mark.parametrize("kind,mean,P,n,agg", HOST_CASES)
def test_dropin_host_path(tmp_path, oracle_lib, kind, mean, P, n, agg):
    M, q = 24, 8
    X, Y, Q = dropin_problem(kind, P, n, M, 1000 * kind + 100 * mean + 10 * P + n)
    # (the crossover: acqui::EI's f+ is one query_batch over the samples, which a host-resident model hands to the device from
    # 4096 point-sample pairs on — there is none here)
    got = run_driver(tmp_path, kind, mean, X, Y, Q, q, agg, env={"LIMBO_AMD_MIN_N_FOR_GPU": str(1 << 20), "LIMBO_AMD_HOST_BATCH_CROSSOVER": str(1 << 40)})
    got["_n"] = n
    assert n == 0 or got["host_resident"][0] == 1
    Sig, mu, fplus = dropin_reference(oracle_lib, kind, mean, X, Y, Q, agg)
    check_dropin(got, Sig, mu, fplus, q, exact_ties=(n == 0))
    if n == 0:  # EI is 0 everywhere without samples (acqui/ei.hpp): every round of the helper is a tie
        assert np.array_equal(got["ei"], np.arange(q))
