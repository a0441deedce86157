"""The CPU yardstick of sample removal (include/gpe_remove.h): the column sweep in numpy, and the definition it must reproduce.

remove(L, R): sweep the columns c = min R .. n - 1 of the factor L of an n-sample model.  A column in R: its part below the
diagonal becomes an update vector, row and column c disappear.  A kept column: one Givens rotation with every live vector,
chosen from (L[c, c], u[c]) — r = hypot(d, u), cs = d / r, sn = u / r, rows c .. n - 1 of the pair become
(cs x + sn y, -sn x + cs y) — which zeroes u[c] and leaves a positive diagonal.  What remains in the kept rows and columns is
chol(K[S, S]), S the kept set in its original order: refactor(K, R).
"""
import numpy as np


def kept(n, R):
    m = np.ones(n, bool)
    m[np.asarray(sorted(R), int)] = False
    return np.flatnonzero(m)


def remove(L, R):
    L = np.array(L, dtype=np.float64)
    n = L.shape[0]
    Rs = set(int(r) for r in R)
    assert len(Rs) == len(list(R)) and all(0 <= r < n for r in Rs)
    U = []
    for c in range(min(Rs), n):
        if c in Rs:
            u = np.zeros(n)
            u[c + 1:] = L[c + 1:, c]
            U.append(u)
            continue
        for u in U:
            d, uc = L[c, c], u[c]
            r = np.hypot(d, uc)
            cs, sn = d / r, uc / r
            x, y = L[c:, c].copy(), u[c:].copy()
            L[c:, c] = cs * x + sn * y
            u[c:] = -sn * x + cs * y
            u[c] = 0.0
    S = kept(n, Rs)
    return np.tril(L[np.ix_(S, S)])


def refactor(K, R):
    S = kept(K.shape[0], R)
    return np.linalg.cholesky(K[np.ix_(S, S)])


def se_ard_kernel(X, noise, theta=None):
    """SE-ARD with log length scales theta[:D] and log sigma_f theta[D] (zeros: unit scales), + (noise + 1e-8) I."""
    n, D = X.shape
    th = np.zeros(D + 1) if theta is None else np.asarray(theta, float)
    Z = X / np.exp(th[:D])
    d2 = np.maximum(((Z[:, None, :] - Z[None, :, :]) ** 2).sum(-1), 0.0)
    return np.exp(2.0 * th[D]) * np.exp(-0.5 * d2) + (noise + 1e-8) * np.eye(n)
