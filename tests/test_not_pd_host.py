"""The inputs of tests/test_gpu_not_pd.py on the CPU: tests/not_pd_cases.py builds every (N, j) the GPU file uses and asserts, with
LAPACK in float64, that pivot j is the first non-positive one with a margin no rounding can cross; the C oracle — another
implementation of gp.hpp:550-571 — is then held to the contract of include/gpe.h on the device-kernel cases: status j + 1, a
log-likelihood that is not finite, and a clean factorisation after the noise is made positive again.  (The oracle's add_sample
reports no pivot, as the reference never does: for the appends the reference is the builder's number.)"""
import numpy as np
import pytest

from tests import not_pd_cases as C
from tests.util import new_gp


@pytest.mark.parametrize("N,j,P", C.ALL_CASES, ids=lambda v: str(v))
def test_first_non_positive_pivot_is_pivot_j(N, j, P):
    X, om, th, noise, K = C.case(N, j, P=P)
    rec = C.info(N, j, P=P)
    assert K.shape == (N, N) and om.shape == (N, P) and rec.status == j + 1
    assert rec.min_pivot_before >= C.PIVOT_MIN and rec.pivot <= C.PIVOT_MAX
    if j > 0:
        assert noise == C.NOISE_BAD and abs(rec.pivot - (0.99 + 1e-8 - 1.0 / (0.99 + 1e-8))) < 1e-2
        dup = [i for i in range(j) if np.array_equal(X[i], X[j])]
        assert len(dup) == 1
    else:
        assert noise == C.NOISE_BAD_FIRST and abs(rec.pivot + 0.5) < 1e-7
    # the same samples with positive noise: positive definite, so the handle-reuse checks have a factorisation to compare
    assert C.lapack_info(C.good_K(X)) == 0


@pytest.mark.parametrize("n0,q,dup_at", C.APPEND_CASES, ids=lambda v: str(v))
def test_append_cases_fail_at_the_first_copy(n0, q, dup_at):
    X0, V, om, th, noise, status = C.append_case(n0, q, dup_at)
    assert status == n0 + min(dup_at) + 1 and om.shape[0] == n0 + q
    assert C.lapack_info(C.kernel(X0, noise)) == 0  # the model the points are appended to is positive definite
    Xall = np.vstack([X0, V])
    assert C.lapack_info(C.kernel(Xall, noise)) == status
    assert C.lapack_info(C.good_K(Xall)) == 0


@pytest.mark.parametrize("N,j,g", [(N, j, g) for N, j, G in C.BATCH_CASES + C.BATCH_PANELS for g in range(G)])
def test_batch_members_without_the_duplicate_are_positive_definite(N, j, g):
    Xg = C.member_X(N, j, g)
    X = C.case(N, j)[0]
    assert np.array_equal(np.delete(Xg, j, 0), np.delete(X, j, 0)) and not np.array_equal(Xg[j], X[j])
    assert C.lapack_info(C.kernel(Xg, C.NOISE_BAD)) == 0


@pytest.mark.parametrize("N,j,P", C.ORACLE_CASES, ids=lambda v: str(v))
def test_oracle_reports_the_pivot_and_recovers(oracle_lib, N, j, P):
    X, om, th, noise, K = C.case(N, j, P=P)
    h = new_gp(oracle_lib, 0, X, om, th, noise)
    assert h.compute() == j + 1
    assert not np.isfinite(h.log_lik())
    h.set_kernel(0, th, C.NOISE_GOOD)
    assert h.compute() == 0
    assert np.isfinite(h.log_lik())
    h.close()
