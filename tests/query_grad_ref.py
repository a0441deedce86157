"""numpy / LAPACK reference of the posterior's gradient in the query point (include/gpe_query_grad.h) — the checker of
tests/test_query_grad_host.py, tests/test_gpu_query_grad.py and the C++ drop-in's tests.  Never the engine.

For a model (X, obs_mean, kernel kind, log-theta as in include/gpe.h, noise) and points V, with k_i = k(v, x_i):
    kta  = k^T alpha_p                      dkta = sum_i alpha_ip dk_i/dv
    var  = k(v, v) - k^T K^-1 k             dvar = -2 sum_i (K^-1 k)_i dk_i/dv
    dk(v, x)/dv = g(z) Mm (v - x),  z = (v - x)^T Mm (v - x)
Mm and g per kind: `mm_matrix`, `g_of_z`.  Two independent routes to alpha and K^-1 k:
    route "chol"   LAPACK dpotrf / dpotrs on K = k(X, X) + (noise + 1e-8) I (kernel.hpp:81-84)
    route "lu"     LAPACK dgetrf / dgetrs with two steps of iterative refinement, the residual in extended precision
`python -m tests.query_grad_ref` prints their disagreement on the shapes the GPU tests use."""
import numpy as np
import scipy.linalg as sla

from oracle import np_oracle as O

LD = np.longdouble
NOISE = 0.01


def ells(D):
    """length scales 0.3 .. 1.0"""
    return np.linspace(0.3, 1.0, D) if D > 1 else np.array([0.6])


def theta_of(kind, D, lam_cols=0, seed=0):
    """log-theta in the engine's order (gpe.h): SE-ARD log ell_1..D [, Lambda column-major, not in log-space], log sigma_f = 0;
    the isotropic kinds log l, log sigma_f = 0"""
    if kind != O.SE_ARD:
        return np.log([0.7, 1.0])
    lam = np.random.default_rng(1000 + seed).uniform(-0.5, 0.5, D * lam_cols)
    return np.concatenate([np.log(ells(D)), lam, [0.0]])


def make_problem(N, D, P, seed):
    """X uniform in [0, 1]^D, y = sin(3 X.u) + 0.1 N(0, 1) centred (tests/sparse_ref.make_problem's)"""
    rng = np.random.default_rng(seed)
    X = rng.random((N, D))
    Y = np.stack([np.sin(3.0 * X @ rng.random(D)) + 0.1 * rng.standard_normal(N) for _ in range(P)], axis=1)
    return X, Y - Y.mean(axis=0)


def make_points(X, M, seed):
    """M points uniform in [0, 1]^D; the first four (as many as fit) training points verbatim (z = 0) and, from six points on,
    the last point a copy of the fifth"""
    rng = np.random.default_rng(seed)
    V = rng.random((M, X.shape[1]))
    nt = min(4, M)
    V[:nt] = X[rng.permutation(X.shape[0])[:nt]]
    if M >= 6:
        V[M - 1] = V[4]
    return V


def mm_matrix(kind, theta, D):
    theta = np.asarray(theta, float)
    if kind == O.SE_ARD:
        Mm = np.diag(np.exp(theta[:D]) ** -2.0)
        if theta.size > D + 1:
            k = (theta.size - 1) // D - 1
            A = theta[D:D + D * k].reshape(k, D).T  # squared_exp_ard.hpp:100-102: _A(i, j) = p((j + 1) D + i)
            Mm = Mm + A @ A.T
        return Mm
    return np.eye(D) * np.exp(theta[0]) ** -2.0


def sf2_of(kind, theta):
    return np.exp(2.0 * np.asarray(theta, float)[-1])


def g_of_z(kind, z, sf2):
    z = np.maximum(z, 0.0)
    if kind in (O.SE_ARD, O.EXP):
        return -sf2 * np.exp(-0.5 * z)
    if kind == O.MATERN52:
        s = np.sqrt(5.0 * z)
        return -(5.0 / 3.0) * sf2 * (1.0 + s) * np.exp(-s)
    return -3.0 * sf2 * np.exp(-np.sqrt(3.0 * z))


def k_of_z(kind, z, sf2):
    z = np.maximum(z, 0.0)
    if kind in (O.SE_ARD, O.EXP):
        return sf2 * np.exp(-0.5 * z)
    if kind == O.MATERN52:
        s = np.sqrt(5.0 * z)
        return sf2 * (1.0 + s + (5.0 / 3.0) * z) * np.exp(-s)
    s = np.sqrt(3.0 * z)
    return sf2 * (1.0 + s) * np.exp(-s)


def dk_dv(kind, theta, v, x):
    """one pair: dk(v, x)/dv (what the drop-in's host function computes)"""
    d = np.asarray(v, float) - np.asarray(x, float)
    Mm = mm_matrix(kind, theta, d.size)
    return g_of_z(kind, d @ Mm @ d, sf2_of(kind, theta)) * (Mm @ d)


def solver_chol(K):
    cf = sla.cho_factor(K, lower=True)
    return lambda B: sla.cho_solve(cf, B)


def solver_lu(K, steps=2):
    lu, Kl = sla.lu_factor(K), K.astype(LD)

    def solve(B):
        x = sla.lu_solve(lu, B)
        for _ in range(steps):  # iterative refinement, the residual in extended precision
            x = x + sla.lu_solve(lu, (B.astype(LD) - Kl @ x.astype(LD)).astype(np.float64))
        return x

    return solve


def reference(kind, X, om, theta, noise, V, route="chol", chunk=128):
    """(kta (M, P), var (M), dkta (M, D, P), dvar (M, D)) — no mean functor, no clamp, no + noise"""
    X, V, om = np.asarray(X, float), np.asarray(V, float), np.asarray(om, float).reshape(X.shape[0], -1)
    N, D = X.shape
    M, P = V.shape[0], om.shape[1]
    K = O.kernel_matrix(kind, X, theta, noise)
    solve = solver_chol(K) if route == "chol" else solver_lu(K)
    Mm, sf2 = mm_matrix(kind, theta, D), sf2_of(kind, theta)
    alpha = solve(om)
    kta, var = np.zeros((M, P)), np.zeros(M)
    dkta, dvar = np.zeros((M, D, P)), np.zeros((M, D))
    for m0 in range(0, M, chunk):
        v = V[m0:m0 + chunk]
        diff = v[:, None, :] - X[None, :, :]           # (m, N, D)
        md = diff @ Mm                                 # Mm (v - x), Mm symmetric
        z = np.einsum("mnd,mnd->mn", md, diff)
        k, g = k_of_z(kind, z, sf2), g_of_z(kind, z, sf2)
        w = solve(k.T).T                            # (m, N): K^-1 k
        kta[m0:m0 + chunk] = k @ alpha
        var[m0:m0 + chunk] = sf2 - np.einsum("mn,mn->m", k, w)
        gd = g[:, :, None] * md                        # dk_i/dv
        dkta[m0:m0 + chunk] = np.einsum("mnd,np->mdp", gd, alpha)
        dvar[m0:m0 + chunk] = -2.0 * np.einsum("mnd,mn->md", gd, w)
    return kta, var, dkta, dvar


# (kind, N, D, P, Lambda columns) of tests/test_gpu_query_grad.py's parity cases; the edge sizes and the real size follow
GPU_SHAPES = [
    (O.SE_ARD, 300, 3, 1, 0), (O.SE_ARD, 1100, 6, 2, 0), (O.SE_ARD, 700, 20, 1, 0), (O.SE_ARD, 600, 5, 1, 2), (O.MATERN52, 520, 2, 1, 0),
    (O.MATERN32, 300, 3, 1, 0), (O.EXP, 300, 3, 1, 0),
] + [(O.SE_ARD, n, 6, 1, 0) for n in (200, 255, 256, 257, 1024, 1100)] + [(O.SE_ARD, 4096, 6, 1, 0)]


def routes_disagreement(kind, N, D, P, lam, M=64, seed=5):
    X, om = make_problem(N, D, P, seed)
    th = theta_of(kind, D, lam, seed)
    V = make_points(X, M, seed + 1)
    a = reference(kind, X, om, th, NOISE, V, "chol")
    b = reference(kind, X, om, th, NOISE, V, "lu")
    return [float(np.max(np.abs(p - q))) for p, q in zip(a, b)]


if __name__ == "__main__":
    for shape in GPU_SHAPES:
        print(shape, ["%.2e" % d for d in routes_disagreement(*shape)])
