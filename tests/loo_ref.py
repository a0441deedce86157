"""Leave-one-out cross-validation of the exact GP in numpy / LAPACK: the checker of tests/test_gpu_loo_cv.py (GPU) and of
tests/test_loo_host.py (CPU, where it is held against the C oracle).  Neither the engine nor the C oracle: built on
oracle/np_oracle.py (gp_fit, inv_kernel, kernel_grad_tensor, obs_mean_data), the literal form of the reference's
model/gp.hpp:339-402.  With kappa = diag(K^-1):

  value     sum_{i,p} (-1/2 alpha_ip^2 / kappa_i + 1/2 log kappa_i - 1/2 log 2 pi)                               (gp.hpp:346-348)
  gradient  per hyper-parameter j, Z = K^-1 dK_j:
            g_j = sum_{i,p} (alpha_ip (Z alpha)_ip - 1/2 (1 + alpha_ip^2 / kappa_i) (Z K^-1)_ii) / kappa_i       (gp.hpp:389-393)
            with optimize_noise one more entry, dK = 2 noise I                                                  (kernel.hpp:86-96)
  weights   u = K^-1 (alpha / kappa),  c_i = sum_p 1/2 (1 + alpha_ip^2 / kappa_i) / kappa_i,
            W = sum_p sym(u_p alpha_p^T) - K^-1 diag(c) K^-1        (what gpe_get_loo_weights returns: g_j = sum W o dK_j)

The gradient is NOT computed through W (loo_grad: one dense N^3 product per parameter, as the reference does); loo_weights is a
second function, and tests/test_loo_host.py holds the two against each other.

Inputs: the recipe of tests/test_gpu_parity.py::test_gpu_loo_cv_vs_oracle (X uniform in [0, 1]^D, y_p = cos((p + 1) sum x) + 0.05
N(0, 1), noise 0.02, theta uniform in [-0.5, 0.3]; cond(K^-1) 2e4 .. 1.3e5 there).  References are cached per case in this module
and are not to be modified by their users."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from oracle import np_oracle as O

NOISE = 0.02
_cache = {}


def n_theta(kind, D):
    return D + 1 if kind == O.SE_ARD else 2


def make_problem(N, D, P, kind, n_thetas=1, seed=None):
    """(X, Y, thetas): test_gpu_loo_cv_vs_oracle's inputs (its seed N + 31 D, its order of draws); further thetas follow the first."""
    rng = np.random.default_rng(N + 31 * D if seed is None else seed)
    X = rng.uniform(0, 1, size=(N, D))
    Y = np.stack([np.cos((p + 1) * X.sum(axis=1)) + 0.05 * rng.normal(size=N) for p in range(P)], axis=1)
    thetas = [rng.uniform(-0.5, 0.3, size=n_theta(kind, D)) for _ in range(n_thetas)]
    return X, Y, thetas


def loo_value(Kinv, alpha):
    kappa = np.diag(Kinv)[:, None]
    return float(np.sum(-0.5 * alpha * alpha / kappa + 0.5 * np.log(kappa) - 0.5 * np.log(2.0 * np.pi)))


def loo_grad(Kinv, alpha, dKs):
    """dKs: an iterable of N x N matrices dK / d theta_j."""
    kappa = np.diag(Kinv)[:, None]
    half = 0.5 * (1.0 + alpha * alpha / kappa)
    g = []
    for dK in dKs:
        Z = Kinv @ dK
        zk = np.einsum("ik,ki->i", Z, Kinv)[:, None]  # diag(Z K^-1)
        g.append(float(np.sum((alpha * (Z @ alpha) - half * zk) / kappa)))
    return np.array(g)


def loo_weights(Kinv, alpha):
    kappa = np.diag(Kinv)[:, None]
    u = Kinv @ (alpha / kappa)
    c = np.sum(0.5 * (1.0 + alpha * alpha / kappa) / kappa, axis=1)
    ua = u @ alpha.T
    return 0.5 * (ua + ua.T) - (Kinv * c[None, :]) @ Kinv


def dK_list(kind, X, theta, noise, optimize_noise):
    G = O.kernel_grad_tensor(kind, X, theta)
    dKs = [G[t] for t in range(G.shape[0])]
    if optimize_noise:
        dKs.append(2.0 * noise * np.eye(X.shape[0]))
    return dKs


def reference(kind, X, obs_mean, theta, noise, optimize_noise, want_W=False, want_lik_grad=False):
    """value, gradient (len(theta) + optimize_noise entries), K^-1, optionally W, and optionally the log-likelihood and its gradient
    (oracle/np_oracle.py: log_lik, log_lik_grad) of the same fit."""
    K, L, alpha = O.gp_fit(kind, X, obs_mean, theta, noise)
    Kinv = O.inv_kernel(L)
    dKs = dK_list(kind, X, theta, noise, optimize_noise)
    r = SimpleNamespace(Kinv=Kinv, alpha=alpha, value=loo_value(Kinv, alpha), grad=loo_grad(Kinv, alpha, dKs), W=None, lik=None,
                        lik_grad=None)
    if want_W:
        r.W = loo_weights(Kinv, alpha)
    if want_lik_grad:
        r.lik = float(O.log_lik(L, obs_mean, alpha))
        r.lik_grad = O.log_lik_grad(kind, X, theta, noise, L, alpha, optimize_noise)
    return r


def cached(key, build):
    """The reference of a case, computed once per process; `key` names the case."""
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]
