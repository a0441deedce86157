"""gpe_add_samples (include/gpe_append.h): a batch of samples appended to a fitted model in one blocked update.

The yardstick of every number is the CPU oracle, which has no batched call: the same points go in through q single add_sample
calls (and, where oracle/_ref is present, through the reference's own GP::add_sample loop).  The tolerances are the project's
existing ones for appended rows at noise 0.01 (test_gpu_configs.py::test_gpu_c5_add_sample_loop, parity_checks.py): L 1e-10 of
max|L|, alpha 1e-7 relative, log-lik TOL_LL, mu TOL_MU, sigma^2 TOL_VAR (sigma^2 including + noise)."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from limbo_amd import _capi, synth
from oracle import binding as OB
from oracle import np_oracle as O
from tests import parity_checks as PC
from tests.util import new_gp, relerr, relerr_norm

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NOISE = 0.01
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -2, -5

# kernel -> (kind, D, P, Lambda columns)
KERNELS = {"p4": (O.SE_ARD, 3, 4, 0), "se": (O.SE_ARD, 6, 1, 0), "m52": (O.MATERN52, 3, 2, 0), "lam": (O.SE_ARD, 4, 3, 1), "wide": (O.SE_ARD, 21, 1, 0)}


def _theta(kname, seed=0):
    kind, D, _, lam = KERNELS[kname]
    if kind != O.SE_ARD:
        return np.zeros(2)
    th = np.zeros(D + D * lam + 1)
    if lam:  # the entries of Lambda are not in log-space (squared_exp_ard.hpp:100-102)
        th[D:D + D * lam] = np.random.default_rng(77 + seed).uniform(-0.5, 0.5, size=D * lam)
    return th


def _problem(kname, n, seed, dup=None):
    """U[0, 1]^D inputs, smooth targets plus 5 % noise."""
    _, D, P, _ = KERNELS[kname]
    rng = np.random.default_rng(1000 + seed)
    X = rng.uniform(0, 1, size=(n, D))
    if dup:
        for dst, src in dup:
            X[dst] = X[src]
    f = np.stack([np.sin(3.0 * X.sum(axis=1) / np.sqrt(D) + p) + 0.5 * np.cos(2.0 * X[:, 0] + p) for p in range(P)], axis=1)
    Y = f + 0.05 * np.std(f, axis=0) * rng.normal(size=f.shape)
    return X, Y


def _fit(lib, kname, X, Y, n0, th):
    """set_data + compute on the first n0 samples (an empty handle with its kernel set for n0 == 0)."""
    kind = KERNELS[kname][0]
    if n0 == 0:
        h = _capi.Handle(lib)
        h.set_kernel(int(kind), th, NOISE)
        return h
    om0, _ = synth.obs_mean_data(Y[:n0])
    h = new_gp(lib, kind, X[:n0], om0, th, NOISE)
    assert h.compute() == 0
    return h


def _append_loop(h, X, om, n0, n1):
    """n1 - n0 single add_sample calls, each with the leading rows of the same obs_mean."""
    for n in range(n0, n1):
        assert h.add_sample(X[n], om[: n + 1]) == 0


def _query_points(X, n0, n1, D, seed):
    Xq = np.random.default_rng(5000 + seed).uniform(0, 1, size=(64, D))
    Xq[0] = X[0 if n0 == 0 else n0 // 2]  # two training points, one of them a new point
    Xq[1] = X[n1 - 1]
    return Xq


def _compare(g, o, Xq, mean, tag=""):
    """L, alpha, log-lik, mu, sigma^2 of the engine handle g against the oracle handle o in the same state."""
    assert g.nb_samples() == o.nb_samples()
    Lg, Lo = g.get_L(), o.get_L()
    eL = float(np.max(np.abs(Lg - Lo)) / np.max(np.abs(Lo)))
    ea = relerr_norm(g.get_alpha(), o.get_alpha())
    llg, llo = g.log_lik(), o.log_lik()
    kg, vg = g.query_batch(Xq)
    ko, vo = o.query_batch(Xq)
    mg, sg = synth.finish_query(kg, vg, mean, NOISE)
    mo, so = synth.finish_query(ko, vo, mean, NOISE)
    emu, es2 = relerr(mg, mo, floor=1e-3), relerr(sg, so)
    print(f"{tag}: L {eL:.2e}  alpha {ea:.2e}  ll {abs(llg - llo) / abs(llo):.2e}  mu {emu:.2e}  sigma^2 {es2:.2e}")
    assert np.isfinite(eL) and eL <= 1e-10, eL
    assert ea < 1e-7, ea
    assert abs(llg - llo) <= PC.TOL_LL * abs(llo), (llg, llo)
    assert emu < PC.TOL_MU, emu
    assert es2 < PC.TOL_VAR, es2


def _appended_pair(engine_lib, oracle_lib, kname, n0, q, seed, dup=None, cap_exact=False):
    """(engine handle after ONE add_samples, oracle handle after q add_sample calls, X, Y, obs_mean, mean, theta)."""
    n1 = n0 + q
    X, Y = _problem(kname, n1, seed, dup)
    om, mean = synth.obs_mean_data(Y)
    th = _theta(kname, seed)
    g = _fit(engine_lib, kname, X, Y, n0, th)
    o = _fit(oracle_lib, kname, X, Y, n0, th)
    if cap_exact:
        assert n0 % 64 == 0  # set_data allocates n0 rounded up to 64: nothing to spare, the batch forces the capacity to grow
    e0 = g.epoch()
    assert g.add_samples(X[n0:], om) == 0
    assert g.epoch() != e0
    _append_loop(o, X, om, n0, n1)
    assert g.nb_samples() == n1
    return g, o, X, Y, om, mean, th


def _chunk(engine_lib):
    c = _capi.append_max_chunk(engine_lib)
    assert 1 <= c <= 128
    return c


SE_ROWS = [(256, 1), (300, 7), (320, 64), (317, 64), (450, 128), (500, 130), (500, "2c+3"), (256, 64), (250, 20), (60, 10), (0, 40)]
OTHER = [(k, n0, q) for k in ("m52", "lam", "wide") for (n0, q) in ((317, 64), (500, 130))]
# four outputs: the one-launch small path does not apply (P <= 3), so below one outer panel the points go in by the general
# single append — all of them (100 -> 130), and up to the panel with the block path behind (200 -> 256 -> 280)
OTHER += [("p4", 100, 30), ("p4", 200, 80)]


@pytest.mark.parametrize("kname,n0,q", [("se", n0, q) for (n0, q) in SE_ROWS] + OTHER)
def test_gpu_add_samples_parity(engine_lib, oracle_lib, kname, n0, q):
    """One add_samples against q oracle add_sample calls: q = 1; inside one 64-block, unaligned; a block-aligned start; a batch
    that straddles a 64-block boundary with the first touched block partly old; one that crosses the 256-panel boundary at 512
    (a full-width chunk if the chunk is 128); more than one chunk; a capacity of exactly n0 (256: the batch forces grow_dev);
    the small-path / general boundary; the small path throughout; an empty handle.  SE-ARD D = 6 on every row, Matern-5/2
    (D = 3, P = 2), SE-ARD with one Lambda column (D = 4, P = 3) and D = 21 (the wide kernel build) on two of them."""
    if q == "2c+3":
        q = 2 * _chunk(engine_lib) + 3
    D = KERNELS[kname][1]
    g, o, X, Y, om, mean, th = _appended_pair(engine_lib, oracle_lib, kname, n0, q, seed=n0 + q, cap_exact=(n0, q) == (256, 64))
    Xq = _query_points(X, n0, n0 + q, D, n0)
    _compare(g, o, Xq, mean, f"{kname} ({n0}, {q})")
    if OB.ref_available() and kname == "se" and (n0, q) in ((317, 64), (500, 130)):  # the reference's own add_sample loop
        r = OB.RefGP(O.SE_ARD, D, 1, noise=NOISE)
        r.set_h_params(th)
        r.compute(X[:n0], Y[:n0])
        for n in range(n0, n0 + q):
            r.add_sample(X[n], Y[n])
        Lr = r.matrixL()
        assert np.max(np.abs(g.get_L() - Lr)) <= 1e-10 * np.max(np.abs(Lr))
        assert relerr_norm(g.get_alpha(), r.alpha()) < 1e-7
        mu_r, s2_r = r.query(Xq)
        kg, vg = g.query_batch(Xq)
        mg, sg = synth.finish_query(kg, vg, mean, NOISE)
        assert relerr(mg, np.asarray(mu_r).reshape(mg.shape), floor=1e-3) < PC.TOL_MU
        assert relerr(sg, np.asarray(s2_r).reshape(sg.shape)) < PC.TOL_VAR
        r.close()
    g.close()
    o.close()


def test_gpu_add_samples_state_is_usable(engine_lib, oracle_lib):
    """After (317, 64) — rows 317 .. 380: block 4 is partly old, block 5 new — the state serves everything a model serves: one
    more single add_sample, a second add_samples of 5, a batch query of 300 points, the log-likelihood gradient, update_alpha
    with new targets, each against the oracle in the same state.  A stale diagonal-block inverse (an implementation that
    refreshes only the last block) or a wrong K^-1 flag shows here."""
    n0, q, D = 317, 64, 6
    n1 = n0 + q
    extra = 6
    Xall, Yall = _problem("se", n1 + extra, seed=42)
    th = _theta("se")
    g = _fit(engine_lib, "se", Xall, Yall, n0, th)
    o = _fit(oracle_lib, "se", Xall, Yall, n0, th)
    g.compute_inv_kernel()  # a K^-1 that the append must invalidate (gp.hpp:602)
    om, mean = synth.obs_mean_data(Yall[:n1])
    assert g.add_samples(Xall[n0:n1], om) == 0
    _append_loop(o, Xall, om, n0, n1)
    rng = np.random.default_rng(8)
    # the gradient first: it needs K^-1 of the NEW factor
    gg, go = g.log_lik_grad(False), o.log_lik_grad(False)
    assert relerr_norm(gg, go) < PC.TOL_GRAD
    Xq = rng.uniform(0, 1, size=(300, D))
    kg, vg = g.query_batch(Xq)
    ko, vo = o.query_batch(Xq)
    mg, sg = synth.finish_query(kg, vg, mean, NOISE)
    mo, so = synth.finish_query(ko, vo, mean, NOISE)
    assert relerr(mg, mo, floor=1e-3) < PC.TOL_MU and relerr(sg, so) < PC.TOL_VAR
    # one more single sample
    om, mean = synth.obs_mean_data(Yall[: n1 + 1])
    assert g.add_sample(Xall[n1], om) == 0 and o.add_sample(Xall[n1], om) == 0
    _compare(g, o, Xq[:64], mean, "single after batch")
    # a second batch of 5
    om, mean = synth.obs_mean_data(Yall)
    assert g.add_samples(Xall[n1 + 1:], om) == 0
    _append_loop(o, Xall, om, n1 + 1, n1 + extra)
    _compare(g, o, Xq[:64], mean, "second batch")
    gg, go = g.log_lik_grad(False), o.log_lik_grad(False)
    assert relerr_norm(gg, go) < PC.TOL_GRAD
    # new targets on the appended factor
    Y2 = Yall[:, ::-1] * 0.7 + rng.normal(0, 0.05, size=Yall.shape)
    om2, mean2 = synth.obs_mean_data(Y2)
    g.update_alpha(om2)
    o.update_alpha(om2)
    _compare(g, o, Xq[:64], mean2, "update_alpha")
    g.close()
    o.close()


def test_gpu_add_samples_duplicates(engine_lib, oracle_lib):
    """One point repeated inside the batch and one equal to an existing sample: off-diagonal entries of k(V, V) carry no noise,
    as with sequential calls; at noise 0.01 no pivot comes near zero."""
    n0, q = 317, 64
    g, o, X, Y, om, mean, th = _appended_pair(engine_lib, oracle_lib, "se", n0, q, seed=7, dup=[(n0 + 9, n0 + 3), (n0 + 20, 11)])
    _compare(g, o, _query_points(X, n0, n0 + q, 6, 7), mean, "duplicates")
    g.close()
    o.close()


def test_gpu_add_samples_reproducible_and_equal_to_full_compute(engine_lib):
    """Two clones of one state take the same batch: L and alpha are bitwise equal.  And compute() on all n0 + q samples agrees
    with the appended factor to the L tolerance."""
    n0, q = 450, 128
    X, Y = _problem("se", n0 + q, seed=3)
    om, _ = synth.obs_mean_data(Y)
    th = _theta("se")
    g = _fit(engine_lib, "se", X, Y, n0, th)
    a, b = g.clone(), g.clone()
    assert a.add_samples(X[n0:], om) == 0 and b.add_samples(X[n0:], om) == 0
    La, Lb = a.get_L(), b.get_L()
    assert np.array_equal(La, Lb) and np.array_equal(a.get_alpha(), b.get_alpha())
    assert g.nb_samples() == n0  # the clones' source is untouched
    f = new_gp(engine_lib, O.SE_ARD, X, om, th, NOISE)
    assert f.compute() == 0
    Lf = f.get_L()
    assert np.max(np.abs(La - Lf)) <= 1e-10 * np.max(np.abs(Lf))
    assert relerr_norm(a.get_alpha(), f.get_alpha()) < 1e-7
    for h in (g, a, b, f):
        h.close()


def test_gpu_add_samples_contract(engine_lib):
    n0, D = 300, 6
    X, Y = _problem("se", n0 + 8, seed=5)
    om, _ = synth.obs_mean_data(Y)
    th = _theta("se")
    g = _fit(engine_lib, "se", X, Y, n0, th)
    fn = engine_lib.fn("add_samples")
    d = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(_capi._dp)
    omF = np.asfortranarray(om)
    # q = 0: nothing moves, the epoch included
    e0, L0 = g.epoch(), g.get_L()
    assert fn(g._h, d(X[n0:]), 0, D, omF.ctypes.data_as(_capi._dp), 1) == 0
    assert g.epoch() == e0 and np.array_equal(g.get_L(), L0) and g.nb_samples() == n0
    # wrong D, wrong P, q < 0
    assert fn(g._h, d(X[n0:, :5]), 8, 5, omF.ctypes.data_as(_capi._dp), 1) == ERR_ARG
    om2 = np.asfortranarray(np.concatenate([om, om], axis=1))
    assert fn(g._h, d(X[n0:]), 8, D, om2.ctypes.data_as(_capi._dp), 2) == ERR_ARG
    assert fn(g._h, d(X[n0:]), -1, D, omF.ctypes.data_as(_capi._dp), 1) == ERR_ARG
    assert fn(g._h, None, 8, D, omF.ctypes.data_as(_capi._dp), 1) == ERR_ARG
    assert g.nb_samples() == n0 and np.array_equal(g.get_L(), L0)
    # the epoch moves on success
    e0 = g.epoch()
    assert g.add_samples(X[n0:], om) == 0 and g.epoch() != e0 and g.nb_samples() == n0 + 8
    g.close()
    # data but no factor
    s = new_gp(engine_lib, O.SE_ARD, X[:n0], om[:n0], th, NOISE)
    assert fn(s._h, d(X[n0:]), 8, D, omF.ctypes.data_as(_capi._dp), 1) == ERR_STATE
    s.close()
    # a caller-supplied kernel matrix
    k = new_gp(engine_lib, 4, X[:50], om[:50], th, NOISE)
    k.set_K_host(O.kernel_matrix(O.SE_ARD, X[:50], th, NOISE))
    assert k.compute() == 0
    om58 = np.asfortranarray(om[:58])
    assert fn(k._h, d(X[50:58]), 8, D, om58.ctypes.data_as(_capi._dp), 1) == ERR_UNSUPPORTED
    k.close()


def test_gpu_add_samples_launch_economy(engine_lib):
    """One chunk is one pass, whatever its width.  What get_phase_ms reports as `launches` is one record per phase scope of the
    engine (the tail's five launches are one record, every product of the solve is one): their sum for one add_samples at
    n0 = 512 is the same for q = 3 and for q = append_max_chunk().  That the launches themselves do not depend on q is by
    construction (the launch list in DESIGN 3.13 has no term in q within a chunk); this asserts the record count.  No timing."""
    n0 = 512
    ch = _chunk(engine_lib)
    X, Y = _problem("se", n0 + ch, seed=12)
    th = _theta("se")
    g = _fit(engine_lib, "se", X, Y, n0, th)
    counts = []
    for q in (3, ch):
        h = g.clone()
        h.set_profiling(True)
        h.reset_phase_ms()
        om, _ = synth.obs_mean_data(Y[: n0 + q])
        assert h.add_samples(X[n0:n0 + q], om) == 0
        ph = h.get_phase_ms()
        counts.append(sum(v["launches"] for v in ph.values()))
        h.close()
    g.close()
    print("launches:", counts)
    assert counts[0] > 0 and counts[0] == counts[1], counts


def rerun_child():
    """Body of the child process of test_gpu_add_samples_rerun_path (GPE_FLOW_FAULT=1 is read once per process)."""
    eng, orc = _capi.load_engine(), OB.load_oracle()
    g, o, X, Y, om, mean, th = _appended_pair(eng, orc, "se", 317, 64, seed=381)
    assert g.flow_retries() >= 1, g.flow_retries()
    _compare(g, o, _query_points(X, 317, 381, 6, 317), mean, "re-run")
    print("child ok", g.flow_retries())


def test_gpu_add_samples_rerun_path():
    """GPE_FLOW_FAULT=1 makes the first attempt of a one-launch sweep count as timed out (nothing is made to fault): the call's
    re-run repeats the solve, the tail and the sweeps from the untouched inputs, and (317, 64) still gives the oracle's results."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tests.test_gpu_add_samples import rerun_child\n"
            "rerun_child()\n") % str(ROOT)
    env = dict(os.environ, GPE_FLOW_FAULT="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_gpu_dropin_add_samples_equals_the_add_sample_loop(tmp_path):
    """The C++ drop-in on the device (tests/cpp/test_add_samples with `device`: the host threshold is 0): a model::GP of 300
    samples takes add_samples of 40; matrixL(), alpha() and the queries against the same model fed by 40 add_sample calls,
    to the tolerances of the parity test."""
    from tests.test_add_samples_host import build_driver, parse_output, write_input

    n0, q, D = 300, 40, 6
    X, Y = _problem("se", n0 + q, seed=21)
    Q = _query_points(X, n0, n0 + q, D, 21)[:16]
    f = tmp_path / "in.txt"
    write_input(f, 0, 0, X, Y, n0, Q)
    r = subprocess.run([str(build_driver()), str(f), "device"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = parse_output(r.stdout)
    a, b = out["batch"], out["loop"]
    n1 = n0 + q
    assert a["n"] == n1 and b["n"] == n1 and a["status"][0] == 0 and b["status"][0] == 0
    La, Lb = a["L"].reshape(n1, n1, order="F"), b["L"].reshape(n1, n1, order="F")
    assert np.all(np.triu(La, 1) == 0.0)
    assert np.max(np.abs(La - Lb)) <= 1e-10 * np.max(np.abs(Lb))
    assert relerr_norm(a["alpha"], b["alpha"]) < 1e-7
    assert abs(a["log_lik"][0] - b["log_lik"][0]) <= PC.TOL_LL * abs(b["log_lik"][0])
    assert relerr(a["mu"], b["mu"], floor=1e-3) < PC.TOL_MU and relerr(a["sigma"], b["sigma"]) < PC.TOL_VAR
    assert np.max(np.abs(out["multi_batch"] - out["multi_loop"])) <= 1e-8 * max(1.0, np.max(np.abs(out["multi_loop"])))
