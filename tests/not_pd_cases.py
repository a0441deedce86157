"""Kernel matrices whose FIRST non-positive Cholesky pivot is known exactly: the inputs of tests/test_not_pd_host.py (CPU, the C
oracle) and tests/test_gpu_not_pd.py (the engine).  include/gpe.h promises that a factorising call returns 0 or the 1-based index
of that pivot; these cases make the index a fact about the input instead of a property of a schedule.

case(N, j):  X uniform in [0, 1]^D with X[j] = X[i] for one i < j; SE-ARD, log l = -3 (l = 0.05: K is nearly diagonal), sigma_f = 1,
noise = -0.01 (gpe_set_kernel takes any double).  Every diagonal entry is 1 - 0.01 + 1e-8 = 0.99, rows i and j of K differ only on
the diagonal (K[i, j] = 1: no noise off the diagonal, kernel.hpp:83), so pivot j is 0.99 - 1 / 0.99 = -0.0201 up to the little the
other samples contribute, and the pivots before j stay far from zero.  j = 0: noise = -1.5, K[0, 0] = -0.5, no duplicate.

The builder ASSERTS the condition, with LAPACK in float64 on the leading blocks: every pivot before j >= 0.01 and pivot j <= -0.01
(pivot = the diagonal entry of the Schur complement, i.e. the squared diagonal of the factor where it exists).  Rounding (~1e-13)
cannot move a pivot across either bound, so the status of a correct factorisation in ANY summation order is exactly j + 1.  A seed
that does not meet the condition is to be changed; the condition is not.

append_case(n0, q, dup_at): n0 distinct samples (K = chol-able under the same negative noise: no duplicate, nearly diagonal, 0.99 on
the diagonal) and q new points of which those at positions dup_at copy an existing sample: appended to a model of the n0, the first
copy's pivot is the first non-positive one, status n0 + min(dup_at) + 1.  The full (n0 + q) matrix is checked like a case.

Results are cached per argument tuple and are not to be modified by their users."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from oracle import np_oracle as O

LOG_ELL = -3.0
NOISE_BAD = -0.01
NOISE_BAD_FIRST = -1.5  # j = 0
NOISE_GOOD = 0.01
PIVOT_MIN = 0.01   # every pivot before j is at least this
PIVOT_MAX = -0.01  # pivot j is at most this
_cache = {}

# ---- the cases of tests/test_gpu_not_pd.py, (N, j, P), smallest first -------------------------------------------------------
# one data-flow launch that generates K itself: all four positions of a 4-column group, both sides of a 64-block and of a
# 256-column edge, the last full column, the first and the last column of the ragged block (520 = 8 x 64 + 8; 704 = 11 x 64)
ONE_LAUNCH = [(520, j, 1) for j in (0, 1, 2, 3, 63, 64, 255, 256, 511, 512, 519)] + \
             [(704, j, 1) for j in (0, 1, 2, 3, 63, 64, 255, 256, 703)]
HOST_K = [(520, 0, 1), (520, 300, 1), (520, 519, 1)]
MANY_REPORTERS = [(1792, 5, 1), (1792, 64, 1), (1792, 1791, 1)]  # up to 27 diagonal blocks behind the failing one
# GPE_TAIL_MAX=512: tall launch over columns 0 .. 1023, one update, closing launch 1024 .. 1343
TALL = [(1344, j, 2) for j in (70, 1023, 1024, 1343)]
# GPE_TAIL_MAX=512 GPE_TALL=0: 256-column panels to 1024, closing launch behind them; 1407 = 21 x 64 + 63
PANELS = [(1344, 300, 1), (1344, 1023, 1), (1344, 1100, 1), (1407, 1344, 1), (1407, 1406, 1)]
PANELS_FIRST_BLOCK = [(1344, 5, 1)]  # ... and the block in front of the first panel, which k_diag factors alone
SCHEDULES = [(520, 100, 1), (520, 300, 1), (520, 519, 1)]  # under each of the seven fall-back environments
HP_OBJECTIVE = [(1024, 600, 1)]  # the smallest order whose K^-1 is the recursion's
BATCH_CASES = [(520, 515, 3), (704, 300, 3), (1024, 600, 2)]  # (N, j, members): ragged (K built), batched data-flow launch, objective
BATCH_PANELS = [(520, 5, 3)]  # under GPE_TAIL_MAX=0: a batch by panels, whose first block is k_diag_b's
ORACLE_CASES = sorted(set(ONE_LAUNCH + MANY_REPORTERS + TALL + PANELS + PANELS_FIRST_BLOCK + SCHEDULES + HP_OBJECTIVE))
ALL_CASES = sorted(set(ORACLE_CASES + HOST_K + [(N, j, 1) for N, j, _ in BATCH_CASES + BATCH_PANELS]))
# (n0, q, positions of the copies among the q new points)
APPEND_ONE = [(40, 1, (0,)), (300, 1, (0,))]
APPEND_BLOCK = [(300, 70, (0,)), (300, 70, (37,)), (300, 70, (69,))]
APPEND_CHUNKS = (300, 133, (130,))  # q = gpe_append_max_chunk() + 5: the copy lies in the second chunk
APPEND_POINTWISE = [(40, 20, (7,)), (40, 20, (7, 12))]
APPEND_CASES = APPEND_ONE + APPEND_POINTWISE + APPEND_BLOCK + [APPEND_CHUNKS]


def theta(D):
    return np.concatenate([np.full(D, LOG_ELL), [0.0]])


def observations(X, P):
    Y = np.stack([np.cos((p + 1) * X.sum(axis=1)) for p in range(P)], axis=1)
    return O.obs_mean_data(Y)[0]


def pivots_upto(K, j):
    """(the pivots 0 .. j-1, pivot j) of the symmetric K by LAPACK on the leading blocks, float64."""
    import scipy.linalg as sl

    if j == 0:
        return np.zeros(0), float(K[0, 0])
    L = sl.cholesky(K[:j, :j], lower=True)  # raises LinAlgError if a pivot before j is not positive
    z = sl.solve_triangular(L, K[:j, j], lower=True)
    return np.diag(L) ** 2, float(K[j, j] - z @ z)


def lapack_info(K):
    """dpotrf's own info on the full matrix: 0, or the 1-based order of the first leading minor that is not positive definite."""
    import scipy.linalg.lapack as ll

    return int(ll.dpotrf(np.asfortranarray(K), lower=1)[1])


def check(K, j):
    """The condition on the inputs (see the module docstring).  Returns (smallest pivot before j, pivot j)."""
    before, pj = pivots_upto(K, j)
    lo = float(before.min()) if before.size else np.inf
    assert lo >= PIVOT_MIN, f"a pivot before {j} is {lo}: change the seed"
    assert pj <= PIVOT_MAX, f"pivot {j} is {pj}: change the seed"
    assert lapack_info(K) == j + 1
    return lo, pj


def case(N, j, D=4, P=1, seed=None):
    """X (N x D), om (N x P), theta (D + 1), noise, K (N x N float64, + noise + 1e-8 on the diagonal, for the host-K path): the
    first non-positive pivot of K is pivot j (0-based), so a factorising call returns j + 1."""
    key = ("case", N, j, D, P, seed)
    if key not in _cache:
        assert 0 <= j < N
        rng = np.random.default_rng(1000 * N + j if seed is None else seed)
        X = rng.uniform(0, 1, size=(N, D))
        noise = NOISE_BAD_FIRST if j == 0 else NOISE_BAD
        if j > 0:
            X[j] = X[int(rng.integers(0, j))]
        th = theta(D)
        K = O.kernel_matrix(O.SE_ARD, X, th, noise)
        lo, pj = check(K, j)
        for a in (X, K):
            a.setflags(write=False)
        _cache[key] = SimpleNamespace(N=N, j=j, D=D, P=P, X=X, om=observations(X, P), theta=th, noise=noise, K=K, status=j + 1,
                                      min_pivot_before=lo, pivot=pj)
    c = _cache[key]
    return c.X, c.om, c.theta, c.noise, c.K


def info(N, j, D=4, P=1, seed=None):
    """the cached record of case(...): status, min_pivot_before, pivot besides the five arrays"""
    case(N, j, D, P, seed)
    return _cache[("case", N, j, D, P, seed)]


def kernel(X, noise):
    return O.kernel_matrix(O.SE_ARD, X, theta(X.shape[1]), noise)


def good_K(X):
    """the same samples under NOISE_GOOD: positive definite (a duplicated pair has pivot 1.01 - 1 / 1.01 = 0.0199)"""
    return kernel(X, NOISE_GOOD)


def member_X(N, j, g, D=4):
    """case(N, j)'s samples with row j drawn afresh (per member g) instead of copied: positive definite under NOISE_BAD too, with
    every pivot >= PIVOT_MIN (asserted).  The members of a batch share X except for this row."""
    key = ("member", N, j, g, D)
    if key not in _cache:
        import scipy.linalg as sl

        X = case(N, j, D)[0].copy()
        X[j] = np.random.default_rng(31 * N + 7 * j + g + 1).uniform(0, 1, size=D)
        lo = float(np.min(np.diag(sl.cholesky(kernel(X, NOISE_BAD), lower=True)) ** 2))
        assert lo >= PIVOT_MIN, f"member {g}: a pivot is {lo}: change the seed"
        X.setflags(write=False)
        _cache[key] = X
    return _cache[key]


def append_case(n0, q, dup_at, D=4, P=1, seed=None):
    """X0 (n0 x D), V (q x D), om (n0 + q x P, all rows), theta, noise, status: V[t] copies a row of X0 for t in dup_at (each a
    different one); appended to a model of X0 under `noise`, the first non-positive pivot is n0 + min(dup_at) (0-based)."""
    dup_at = tuple(sorted(dup_at))
    key = ("append", n0, q, dup_at, D, P, seed)
    if key not in _cache:
        rng = np.random.default_rng(7000 * n0 + 13 * q + sum(dup_at) if seed is None else seed)
        X = rng.uniform(0, 1, size=(n0 + q, D))
        src = rng.choice(n0, size=len(dup_at), replace=False)
        for t, i in zip(dup_at, src):
            X[n0 + t] = X[int(i)]
        th = theta(D)
        K = O.kernel_matrix(O.SE_ARD, X, th, NOISE_BAD)
        jf = n0 + dup_at[0]
        check(K, jf)
        X.setflags(write=False)
        _cache[key] = SimpleNamespace(X0=X[:n0], V=X[n0:], X=X, om=observations(X, P), theta=th, noise=NOISE_BAD, status=jf + 1)
    c = _cache[key]
    return c.X0, c.V, c.om, c.theta, c.noise, c.status
