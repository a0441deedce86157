"""gpe_remove_samples (include/gpe_remove.h): samples removed from a fitted model by a blocked update of its factor.

The yardstick of every number is the CPU oracle, fitted FRESH (set_data + compute) on the remaining samples in their original
order: the code under test is never its own yardstick.  The tolerances are those of an updated factor at noise 0.01
(test_gpu_add_samples._compare): L 1e-10 of max|L|, alpha 1e-7 relative, log-lik TOL_LL, mu TOL_MU, sigma^2 TOL_VAR.  The numpy
column sweep of tests/remove_ref.py meets them with three orders of margin on the CPU (tests/test_remove_host.py)."""
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
from tests.test_gpu_add_samples import KERNELS, NOISE, _compare, _problem, _theta
from tests.util import new_gp, relerr, relerr_norm

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -2, -5
_ip = _capi.C.POINTER(_capi._i64)


def _cap(lib):
    c = _capi.remove_max_vectors(lib)
    assert 1 <= c <= 64
    return c


# (n0, R as a function of the cap, what it reaches)
SE_ROWS = {
    "320-first": (320, lambda c: [0]),                 # everything shifts by one across every 64- and 256-boundary
    "320-last": (320, lambda c: [319]),                # tail
    "320-last7": (320, lambda c: list(range(313, 320))),  # tail
    "317-63": (317, lambda c: [63]),                   # either side of a block edge, ragged order
    "317-64": (317, lambda c: [64]),
    "256-first": (256, lambda c: [0]),                 # leaves 255: below one outer panel, a block count that drops
    "450-scattered": (450, lambda c: [5, 64, 65, 300, 449]),  # scattered, adjacent, last
    "500-run": (500, lambda c: list(range(100, 132))),  # contiguous, inside one panel
    "700-11th": (700, lambda c: list(range(0, 700, 11))),  # 64 indices: more than one pass if the cap is 32, three panels
    "600-2cap+3": (600, lambda c: sorted(np.random.default_rng(600).choice(600, 2 * c + 3, replace=False).tolist())),  # pass boundaries
    "300-60": (300, lambda c: sorted(np.random.default_rng(300).choice(300, 60, replace=False).tolist())),  # leaves 240
    "60-small": (60, lambda c: [3, 10]),               # small-path region: any path, same answer
}
assert len(list(range(0, 700, 11))) == 64


def _kept(n0, R):
    m = np.ones(n0, bool)
    m[np.asarray(R, int)] = False
    return np.flatnonzero(m)


def _query_points(X, S, D, seed):
    Xq = np.random.default_rng(5000 + seed).uniform(0, 1, size=(64, D))
    Xq[0] = X[S[0]]  # two training points that stay
    Xq[1] = X[S[-1]]
    return Xq


class _Ref:
    """What the oracle answers in one state, computed once and compared against many times (an object with the getters _compare
    calls; the arrays are never written)."""

    def __init__(self, o, Xq):
        self.n, self.L, self.alpha, self.ll = o.nb_samples(), o.get_L(), o.get_alpha(), o.log_lik()
        self.q = o.query_batch(Xq)
        for a in (self.L, self.alpha) + tuple(self.q):
            a.setflags(write=False)

    nb_samples = lambda self: self.n
    get_L = lambda self: self.L
    get_alpha = lambda self: self.alpha
    log_lik = lambda self: self.ll
    query_batch = lambda self, Xq: self.q


_refs = {}


def _case(oracle_lib, kname, n0, R, seed):
    """(X, Y, theta, kept indices, obs_mean and mean of the kept samples, query points, the oracle's fresh fit on the kept samples)"""
    key = (kname, n0, tuple(R), seed)
    if key not in _refs:
        kind, D = KERNELS[kname][0], KERNELS[kname][1]
        X, Y = _problem(kname, n0, seed)
        th = _theta(kname, seed)
        S = _kept(n0, R)
        om, mean = synth.obs_mean_data(Y[S])
        Xq = _query_points(X, S, D, seed)
        o = new_gp(oracle_lib, kind, X[S], om, th, NOISE)
        assert o.compute() == 0
        _refs[key] = (X, Y, th, S, om, mean, Xq, _Ref(o, Xq))
        o.close()
    return _refs[key]


def _fitted(engine_lib, kname, X, Y, th):
    om0, _ = synth.obs_mean_data(Y)
    g = new_gp(engine_lib, KERNELS[kname][0], X, om0, th, NOISE)
    assert g.compute() == 0
    return g


def _remove_and_compare(engine_lib, oracle_lib, kname, n0, R, how, seed=None, order=None):
    seed = n0 + len(R) if seed is None else seed
    X, Y, th, S, om, mean, Xq, ref = _case(oracle_lib, kname, n0, R, seed)
    g = _fitted(engine_lib, kname, X, Y, th)
    e0 = g.epoch()
    assert g.remove_samples(R if order is None else order, om, how) == 0
    assert g.epoch() != e0 and g.nb_samples() == n0 - len(R)
    _compare(g, ref, Xq, mean, f"{kname} ({n0}, {len(R)} removed, {how})")
    return g


@pytest.mark.parametrize("row", list(SE_ROWS))
def test_gpu_remove_samples_parity_update(engine_lib, oracle_lib, row):
    """how = UPDATE, SE-ARD D = 6 P = 1, the smallest shapes that reach every branch (SE_ROWS), against the oracle's fresh fit."""
    n0, Rf = SE_ROWS[row]
    _remove_and_compare(engine_lib, oracle_lib, "se", n0, Rf(_cap(engine_lib)), "update").close()


@pytest.mark.parametrize("kname", ["m52", "lam", "wide", "p4"])
@pytest.mark.parametrize("row", ["317-64", "450-scattered"])
def test_gpu_remove_samples_parity_other_kernels(engine_lib, oracle_lib, kname, row):
    """Matern-5/2 (D = 3, P = 2), SE-ARD with one Lambda column (D = 4, P = 3: the projection rows must move), D = 21, P = 4."""
    n0, Rf = SE_ROWS[row]
    _remove_and_compare(engine_lib, oracle_lib, kname, n0, Rf(_cap(engine_lib)), "update").close()


@pytest.mark.parametrize("how", ["auto", "recompute"])
@pytest.mark.parametrize("row", list(SE_ROWS))
def test_gpu_remove_samples_path_independence(engine_lib, oracle_lib, row, how):
    """The same twelve rows under AUTO and RECOMPUTE: the same verdicts (against the reference the UPDATE rows shared)."""
    n0, Rf = SE_ROWS[row]
    _remove_and_compare(engine_lib, oracle_lib, "se", n0, Rf(_cap(engine_lib)), how).close()


def test_gpu_remove_samples_index_order(engine_lib, oracle_lib):
    """idx in descending (and in shuffled) order gives the bitwise result of ascending."""
    n0, Rf = SE_ROWS["700-11th"]
    R = Rf(_cap(engine_lib))
    a = _remove_and_compare(engine_lib, oracle_lib, "se", n0, R, "update")
    b = _remove_and_compare(engine_lib, oracle_lib, "se", n0, R, "update", order=R[::-1])
    c = _remove_and_compare(engine_lib, oracle_lib, "se", n0, R, "update", order=np.random.default_rng(1).permutation(R))
    assert np.array_equal(a.get_L(), b.get_L()) and np.array_equal(a.get_alpha(), b.get_alpha())
    assert np.array_equal(a.get_L(), c.get_L()) and np.array_equal(a.get_alpha(), c.get_alpha())
    for h in (a, b, c):
        h.close()


def test_gpu_remove_samples_state_is_usable(engine_lib, oracle_lib):
    """After (450, scattered) the state serves everything a model serves, each against the oracle in the same state: the
    log-likelihood gradient (K^-1 was computed BEFORE the removal: a stale flag shows), the leave-one-out score, a 300-point
    query, add_sample, add_samples of 70, a second remove_samples, update_alpha with new targets.  A stale diagonal-block inverse
    or dirty rows beyond N show here."""
    n0, D, extra = 450, 6, 71
    R = SE_ROWS["450-scattered"][1](0)
    Xall, Yall = _problem("se", n0 + extra, seed=43)
    th = _theta("se")
    S = _kept(n0, R)
    g = _fitted(engine_lib, "se", Xall[:n0], Yall[:n0], th)
    g.compute_inv_kernel()
    g.log_loo_cv()
    Xc, Yc = Xall[S], Yall[S]
    om, mean = synth.obs_mean_data(Yc)
    assert g.remove_samples(R, om, "update") == 0
    o = new_gp(oracle_lib, O.SE_ARD, Xc, om, th, NOISE)
    assert o.compute() == 0
    assert relerr_norm(g.log_lik_grad(False), o.log_lik_grad(False)) < PC.TOL_GRAD
    lg, lo = g.log_loo_cv(), o.log_loo_cv()
    assert abs(lg - lo) <= PC.TOL_LL * abs(lo), (lg, lo)
    rng = np.random.default_rng(9)
    Xq = rng.uniform(0, 1, size=(300, D))
    kg, vg = g.query_batch(Xq)
    ko, vo = o.query_batch(Xq)
    mg, sg = synth.finish_query(kg, vg, mean, NOISE)
    mo, so = synth.finish_query(ko, vo, mean, NOISE)
    assert relerr(mg, mo, floor=1e-3) < PC.TOL_MU and relerr(sg, so) < PC.TOL_VAR
    # one more single sample
    Xc, Yc = np.vstack([Xc, Xall[n0:n0 + 1]]), np.vstack([Yc, Yall[n0:n0 + 1]])
    om, mean = synth.obs_mean_data(Yc)
    assert g.add_sample(Xall[n0], om) == 0 and o.add_sample(Xall[n0], om) == 0
    _compare(g, o, Xq[:64], mean, "add_sample after removal")
    # a batch of 70
    Xc, Yc = np.vstack([Xc, Xall[n0 + 1:]]), np.vstack([Yc, Yall[n0 + 1:]])
    om, mean = synth.obs_mean_data(Yc)
    assert g.add_samples(Xall[n0 + 1:], om) == 0
    for n in range(len(Xc) - 70, len(Xc)):
        assert o.add_sample(Xc[n], om[: n + 1]) == 0
    _compare(g, o, Xq[:64], mean, "add_samples after removal")
    # a second removal, the oracle fitted fresh again
    R2 = [0, 63, 64, 255, 256, len(Xc) - 2]
    S2 = _kept(len(Xc), R2)
    Xc, Yc = Xc[S2], Yc[S2]
    om, mean = synth.obs_mean_data(Yc)
    assert g.remove_samples(R2, om, "update") == 0
    o.close()
    o = new_gp(oracle_lib, O.SE_ARD, Xc, om, th, NOISE)
    assert o.compute() == 0
    _compare(g, o, Xq[:64], mean, "second removal")
    assert relerr_norm(g.log_lik_grad(False), o.log_lik_grad(False)) < PC.TOL_GRAD
    # new targets on the updated factor
    Y2 = Yc * 0.7 + rng.normal(0, 0.05, size=Yc.shape)
    om2, mean2 = synth.obs_mean_data(Y2)
    g.update_alpha(om2)
    o.update_alpha(om2)
    _compare(g, o, Xq[:64], mean2, "update_alpha")
    g.close()
    o.close()


def test_gpu_remove_samples_sliding_window(engine_lib, oracle_lib):
    """n = 300, twenty rounds of add_sample + remove_samples([0]); the end state against the oracle on the final 300 points."""
    n, rounds = 300, 20
    X, Y = _problem("se", n + rounds, seed=77)
    th = _theta("se")
    g = _fitted(engine_lib, "se", X[:n], Y[:n], th)
    for t in range(rounds):
        om, _ = synth.obs_mean_data(Y[t:n + t + 1])
        assert g.add_sample(X[n + t], om) == 0
        om, mean = synth.obs_mean_data(Y[t + 1:n + t + 1])
        assert g.remove_samples([0], om, "update") == 0
    assert g.nb_samples() == n
    o = new_gp(oracle_lib, O.SE_ARD, X[rounds:], om, th, NOISE)
    assert o.compute() == 0
    _compare(g, o, _query_points(X, np.arange(rounds, n + rounds), 6, 77), mean, "sliding window")
    g.close()
    o.close()


def test_gpu_remove_samples_reproducible(engine_lib):
    """Two clones take the same removal: L and alpha are bitwise equal, and the source is untouched."""
    n0, Rf = SE_ROWS["700-11th"]
    R = Rf(0)
    X, Y = _problem("se", n0, seed=4)
    th = _theta("se")
    g = _fitted(engine_lib, "se", X, Y, th)
    L0 = g.get_L()
    om, _ = synth.obs_mean_data(Y[_kept(n0, R)])
    a, b = g.clone(), g.clone()
    assert a.remove_samples(R, om, "update") == 0 and b.remove_samples(R, om, "update") == 0
    assert np.array_equal(a.get_L(), b.get_L()) and np.array_equal(a.get_alpha(), b.get_alpha())
    assert g.nb_samples() == n0 and np.array_equal(g.get_L(), L0)
    for h in (g, a, b):
        h.close()


def test_gpu_remove_samples_contract(engine_lib):
    n0 = 300
    X, Y = _problem("se", n0, seed=5)
    th = _theta("se")
    g = _fitted(engine_lib, "se", X, Y, th)
    fn = engine_lib.fn("remove_samples")
    ix = lambda a: np.ascontiguousarray(a, dtype=np.int64).ctypes.data_as(_ip)
    om = np.asfortranarray(synth.obs_mean_data(Y[2:])[0])
    omp = om.ctypes.data_as(_capi._dp)
    # q = 0: nothing moves, the epoch included
    e0, L0 = g.epoch(), g.get_L()
    assert fn(g._h, ix([0]), 0, omp, 1, 0) == 0
    assert g.epoch() == e0 and np.array_equal(g.get_L(), L0) and g.nb_samples() == n0
    # null pointers, q < 0, out of range (both ends), repeated, q >= N, wrong P, unknown how: nothing moves
    om2 = np.asfortranarray(np.concatenate([om, om], axis=1))
    bad = [(None, 2, omp, 1, 1), (ix([0, 1]), 2, None, 1, 1), (ix([0, 1]), -1, omp, 1, 1), (ix([0, n0]), 2, omp, 1, 1),
           (ix([-1, 5]), 2, omp, 1, 1), (ix([7, 7]), 2, omp, 1, 1), (ix(np.arange(n0)), n0, omp, 1, 1),
           (ix([0, 1]), 2, om2.ctypes.data_as(_capi._dp), 2, 1), (ix([0, 1]), 2, omp, 1, 3), (ix([0, 1]), 2, omp, 1, -1)]
    for a in bad:
        assert fn(g._h, *a) == ERR_ARG, a[1:]
        assert g.nb_samples() == n0 and np.array_equal(g.get_L(), L0)
    # at most one more ld x cap matrix alive afterwards (plus the call's scratch: U, one panel's coefficients, the index list)
    cap_rows = 320  # set_data allocates n0 rounded up to 64
    n_before, b_before = _capi.debug_live_buffers(engine_lib)
    e0 = g.epoch()
    assert g.remove_samples([0, 1], om, "update") == 0 and g.epoch() != e0 and g.nb_samples() == n0 - 2
    n_after, b_after = _capi.debug_live_buffers(engine_lib)
    scratch = 8 * _capi.debug_remove_plan(engine_lib, n0, 0, 2)[3]
    print("live buffers:", (n_before, b_before), (n_after, b_after), "scratch", scratch)
    assert b_after - b_before <= 8 * (cap_rows + 64) * cap_rows + scratch + 4096
    assert n_after - n_before <= 2
    g.close()
    # data but no factor
    s = new_gp(engine_lib, O.SE_ARD, X, synth.obs_mean_data(Y)[0], th, NOISE)
    assert fn(s._h, ix([0, 1]), 2, omp, 1, 1) == ERR_STATE
    s.close()
    # a caller-supplied kernel matrix
    k = new_gp(engine_lib, 4, X[:50], synth.obs_mean_data(Y[:50])[0], th, NOISE)
    k.set_K_host(O.kernel_matrix(O.SE_ARD, X[:50], th, NOISE))
    assert k.compute() == 0
    assert fn(k._h, ix([0, 1]), 2, omp, 1, 1) == ERR_UNSUPPORTED
    k.close()


def test_gpu_remove_samples_launch_economy(engine_lib):
    """The launches on the factor do not depend on the number of vectors in a pass: the phase-record count (get_phase_ms's
    `launches`: one record per phase scope) of an UPDATE at n0 = 600 is the same for q = 1 and q = remove_max_vectors() from the
    same i0.  And a tail-only removal records no factor phase at all.  No timing."""
    n0, cap = 600, _cap(engine_lib)
    X, Y = _problem("se", n0, seed=13)
    th = _theta("se")
    g = _fitted(engine_lib, "se", X, Y, th)
    factor = ("potrf_panel", "potrf_update", "potrf_tall", "potrf_tail", "kernel_build")
    counts = []
    for R in ([70], list(range(70, 70 + 2 * cap, 2)), list(range(n0 - 7, n0))):
        h = g.clone()
        h.set_profiling(True)
        h.reset_phase_ms()
        om, _ = synth.obs_mean_data(Y[_kept(n0, R)])
        assert h.remove_samples(R, om, "update") == 0
        ph = h.get_phase_ms()
        counts.append((sum(v["launches"] for v in ph.values()), sum(ph[k]["launches"] for k in factor if k in ph)))
        h.close()
    g.close()
    print("phase records (all, factor):", counts)
    assert counts[0][1] > 0 and counts[0] == counts[1], counts
    assert counts[2][1] == 0, counts
    plan = _capi.debug_remove_plan(engine_lib, n0, 70, 1)
    assert plan[1] == 1 and plan[2] == 2 * 3 - 1  # three panels, the last without rows below, no head in front of panel 0


def rerun_child():
    """Body of the child process of test_gpu_remove_samples_rerun_path (GPE_FLOW_FAULT=1 is read once per process)."""
    eng, orc = _capi.load_engine(), OB.load_oracle()
    X, Y, th, S, om, mean, Xq, ref = _case(orc, "se", 317, [64], 318)
    g = _fitted(eng, "se", X, Y, th)
    r0 = g.flow_retries()
    assert g.remove_samples([64], om, "update") == 0
    assert g.flow_retries() >= r0 + 1 and g.flow_retries() >= 1, (r0, g.flow_retries())
    _compare(g, ref, Xq, mean, "re-run")
    print("child ok", g.flow_retries())


def test_gpu_remove_samples_rerun_path():
    """GPE_FLOW_FAULT=1 makes the first attempt of a one-launch sweep count as timed out (nothing is made to fault): the call's
    re-run repeats alpha's sweeps and the likelihood terms on the updated factor, and (317, {64}) still gives the oracle's results."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tests.test_gpu_remove_samples import rerun_child\n"
            "rerun_child()\n") % str(ROOT)
    env = dict(os.environ, GPE_FLOW_FAULT="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_gpu_dropin_remove_samples_equals_fresh_compute(tmp_path):
    """The C++ drop-in on the device (tests/cpp/test_remove_samples with `device`: the host threshold is 0): a model::GP of 300
    samples drops 40, and a second one its last 5; matrixL(), alpha() and the queries against a fresh compute() on the remaining
    samples."""
    from tests.test_remove_host import build_driver, parse_output

    r = subprocess.run([str(build_driver()), "device"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = parse_output(r.stdout)
    for name, n in (("device-300-40", 260), ("device-300-tail5", 295)):  # (AUTO's choice | tail only: always the update path)
        c = out[name]
        print(name, c)
        assert c["n"] == n and c["L"] <= 1e-10 and c["alpha"] < 1e-7 and c["mu"] < PC.TOL_MU and c["sigma"] < PC.TOL_VAR
