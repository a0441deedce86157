"""CPU tests (no GPU): the problems of tests/test_gpu_high_dim.py and the high-dimensional mpmath goldens are sharp enough to
catch a kernel that drops, truncates or mis-routes a dimension, and they reach the schedule each case claims.

For every problem the GPU tests build (tests/high_dim.py), with numpy only:
  1. dropping the last input dimension, or truncating to the bucket below (the first 16 or 32), moves K by >= 10^3 x the K
     bar of the GPU tests (1e-13 max diag K, the L L^T bar, the looser of the two) and the log-likelihood by >= 10^3 x
     TOL_LL |l|;
  2. the gradient components are pairwise >= 1e-3 apart (relative to the larger), so an output slot fed by the wrong
     accumulator cannot pass a per-component check (problems whose gradient the GPU tests compare with a reference);
  3. the median off-diagonal entry of K is >= 1e-2 sigma_f^2 (K is far from diagonal).
"""
import numpy as np
import pytest

from oracle import np_oracle as O
from tests import high_dim as HD
from tests import parity_checks as PC
from tests.high_dim import check_golden_grad_per_component, high_dim_goldens
from tests.util import load

K_BAR = HD.LLT_BAR


@pytest.mark.parametrize("path", high_dim_goldens(), ids=lambda p: p.stem)
def test_oracle_vs_mpmath_golden_grad_per_component(oracle_lib, path):
    check_golden_grad_per_component(oracle_lib, path)


def test_high_dim_goldens_are_there():
    names = [p.stem for p in high_dim_goldens()]
    assert len(names) == 8 and all(int(n.split("_d")[1].split("_")[0]) >= 16 for n in names), names


def _fit(pb):
    K, L, a = O.gp_fit(pb.kind, pb.X, pb.obs_mean, pb.theta, pb.noise)
    return K, L, a, O.log_lik(L, pb.obs_mean, a)


def _cuts(D):
    """What a wrong kernel could compute instead: the last dimension dropped, the first 16 / 32 (the bucket below) kept."""
    return sorted({D - 1} | {b for b in (16, 32) if b < D}) if D > 1 else []


def check_preconditions(pb, grad):
    K, L, a, ll = _fit(pb)
    sf2 = np.exp(2.0 * pb.theta[-1])
    assert np.median(K[np.tril_indices(pb.N, -1)]) >= 1e-2 * sf2
    bar = 1e3 * K_BAR * np.max(np.diag(K))
    for D2 in _cuts(pb.D):
        K2, _, _, ll2 = _fit(HD.truncated(pb, D2))
        assert np.max(np.abs(K - K2)) >= bar, (pb.D, D2)
        assert abs(ll - ll2) >= 1e3 * PC.TOL_LL * abs(ll), (pb.D, D2, ll, ll2)
    if grad:
        g = O.log_lik_grad(pb.kind, pb.X, pb.theta, pb.noise, L, a, optimize_noise=True)
        d = np.abs(g[:, None] - g[None, :]) / np.maximum(np.abs(g[:, None]), np.abs(g[None, :]))
        np.fill_diagonal(d, np.inf)
        assert np.min(d) >= 1e-3, (np.unravel_index(np.argmin(d), d.shape), float(np.min(d)))


@pytest.mark.parametrize("kind", HD.KINDS, ids=lambda k: HD.KIND_NAMES[k])
def test_sweep_problems_are_sharp(kind):
    for kd, N, D in HD.sweep_cases():
        if kd == kind:
            check_preconditions(HD.problem(kind, N, D), grad=False)


@pytest.mark.parametrize("kind,N,D", HD.big_cases(), ids=lambda v: str(v))
def test_big_sweep_problems_are_sharp(kind, N, D):
    """N = 3392: the GPU test compares 256 sampled columns, so the conditions hold on those columns (K only)."""
    pb = HD.problem(kind, N, D)
    cols = HD.big_columns(N)
    Kc = HD.kernel_columns(kind, pb.X, pb.theta, pb.noise, cols)
    off = np.ones(Kc.shape, bool)
    off[cols, np.arange(cols.size)] = False
    assert np.median(Kc[off]) >= 1e-2 * np.exp(2.0 * pb.theta[-1])
    for D2 in _cuts(D):
        p2 = HD.truncated(pb, D2)
        K2 = HD.kernel_columns(kind, p2.X, p2.theta, pb.noise, cols)
        assert np.max(np.abs(Kc - K2)) >= 1e3 * K_BAR * (np.exp(2.0 * pb.theta[-1]) + pb.noise), (D, D2)


@pytest.mark.parametrize("kind", (O.SE_ARD, O.MATERN52), ids=lambda k: HD.KIND_NAMES[k])
def test_invariance_problems_are_sharp(kind):
    """(Compared bitwise between buckets, not with a reference: no gradient condition.)"""
    for D, _ in HD.INVARIANCE_PAIRS:
        check_preconditions(HD.problem(kind, HD.INVARIANCE_N, D), grad=False)


@pytest.mark.parametrize("case", HD.FULL_CASES, ids=lambda c: c[0])
def test_full_path_problems_are_sharp(case):
    _, kind, N, D, k, P, seed = case
    check_preconditions(HD.full_problem(kind, N, D, k, P, seed), grad=True)


@pytest.mark.parametrize("case", HD.BATCH_CASES, ids=lambda c: c[0])
def test_batch_problems_are_sharp(case):
    _, kind, N, D, G = case
    for g in range(G):
        check_preconditions(HD.batch_problem(kind, N, D, g), grad=True)


def test_growth_problem_is_sharp():
    check_preconditions(HD.growth_problem(), grad=True)


@pytest.mark.parametrize("path", high_dim_goldens(), ids=lambda p: p.stem)
def test_high_dim_golden_problems_are_sharp(path):
    g = load(path)
    N, D = g["X"].shape
    k = (g["theta"].size - 1) // D - 1 if g["kind"] == O.SE_ARD else 0
    pb = HD.SimpleNamespace(kind=g["kind"], X=g["X"], obs_mean=g["obs_mean"], theta=g["theta"], noise=g["noise"], D=D, k=k, N=N)
    check_preconditions(pb, grad=True)


def test_problems_reach_the_schedule_they_claim():
    """gpe_debug_tail_plan (host logic, as test_abi.py::test_schedule_of_the_factorisation_by_size): where K is built."""
    pl = {n: HD.plan(n) for n in (100, 320, 333, 3392)}
    assert pl[100]["t0"] == -1  # k_build_wide builds all of K
    assert pl[320]["t0"] == 0 and 320 % 64 == 0  # one data-flow launch from column 0, every tile generated inside k_tail
    assert pl[333]["t0"] == 0 and pl[333]["n64"] == 320  # generated tiles + a ragged last block from k_build_wide
    assert pl[3392]["t0"] == 768 and pl[3392]["e0"] == 0  # k_build_wide, then the tall and closing launches
    full = {c[0]: c for c in HD.FULL_CASES}
    assert HD.plan(333, 1)["t0"] == 0 and HD.plan(700, 2)["t0"] == 0 and HD.plan(1100, 1)["t0"] == 0
    assert HD.plan(150, 11)["t0"] == 0  # (22 ragged rows + 11 outputs fit the extra strip)
    assert HD.plan(257, 3)["t0"] == 0 and HD.plan(300, 1)["t0"] == 0 and HD.plan(600, 2)["t0"] == 0
    assert HD.plan(200, 1)["t0"] == 0 and len(full) == 10
    # batched: N = 700 is ragged, so k_build_wide<..., true> builds the members' K; N = 640 with G = 5 generates the tiles
    assert HD.plan(700, 1, 3)["t0"] == 0 and 700 % 64 != 0
    assert HD.plan(640, 1, 5)["t0"] == 0 and 640 % 64 == 0
    assert HD.GROWTH[1] < 256 < HD.GROWTH[2]  # add_sample: the small path below 256 samples, the general one above
