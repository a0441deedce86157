"""numpy / LAPACK reference of pathwise posterior draws (include/gpe_pathwise.h) — the checker of tests/test_pathwise_host.py,
tests/test_gpu_pathwise.py and the C++ drop-in's tests.  Never the engine.  Built on tests/query_grad_ref.py.

For a model (X, obs_mean, kernel kind, log-theta, noise), R features (Omega0 (R, Dw), phase (R)), draws W (R, S, P), E (N, S, P):
    f_s(x)  = m(x) + Phi(x) w_s + k(x, X) u_s             u_s = K^-1 (obs_mean - Phi(X) w_s - sqrt(noise + 1e-8) eps_s)
    Phi(x)_r = sqrt(2 sf2 / R) cos(omega_r . x + b_r)       K = k(X, X) + (noise + 1e-8) I
    df_s/dx = -sum_r sqrt(2 sf2 / R) sin(omega_r . x + b_r) omega_r w_rs + sum_i u_is dk(x, x_i)/dx
omega from Omega0 and the hyper-parameters: `scaled_omega`.  Two independent routes to U: LAPACK Cholesky, and LU with two steps of
extended-precision refinement (query_grad_ref.solver_chol / solver_lu).
`python -m tests.pathwise_ref` prints their disagreement on the shapes the GPU tests use."""
import numpy as np

from oracle import np_oracle as O
from tests import query_grad_ref as Q

NOISE = Q.NOISE


def freq_dim(kind, theta, D):
    """Dw: D, and D + k for SE-ARD with k columns of Lambda"""
    theta = np.asarray(theta, float)
    return D + ((theta.size - 1) // D - 1 if kind == O.SE_ARD and theta.size > D + 1 else 0)


def spectral_draws(kind, R, Dw, seed):
    """(Omega0 (R, Dw), phase (R)): the kernel family's spectral law at unit length scale — standard normals (SE-ARD, Exp);
    z sqrt(2 nu / u), u ~ chi^2(2 nu) as a sum of 2 nu squared normals (Matern-nu) — and uniform phases in [0, 2 pi)"""
    rng = np.random.default_rng(seed)
    Om = rng.standard_normal((R, Dw))
    if kind in (O.MATERN52, O.MATERN32):
        dof = 5 if kind == O.MATERN52 else 3
        u = np.sum(rng.standard_normal((R, dof)) ** 2, axis=1)
        Om = Om * np.sqrt(dof / u)[:, None]
    return Om, rng.uniform(0.0, 2.0 * np.pi, R)


def scaled_omega(kind, theta, D, Omega0):
    """omega (R, D): Omega0 / ell (SE-ARD), + Omega0[:, D:] Lambda^T with Lambda; Omega0 / l for the isotropic kinds"""
    theta, Omega0 = np.asarray(theta, float), np.asarray(Omega0, float)
    if kind != O.SE_ARD:
        return Omega0 / np.exp(theta[0])
    om = Omega0[:, :D] / np.exp(theta[:D])
    if theta.size > D + 1:
        k = (theta.size - 1) // D - 1
        A = theta[D:D + D * k].reshape(k, D).T  # (D, k), query_grad_ref.mm_matrix
        om = om + Omega0[:, D:D + k] @ A.T
    return om


def features(kind, theta, D, Omega0, phase, V):
    """(Phi (M, R), the angles (M, R), omega (R, D), the amplitude)"""
    om = scaled_omega(kind, theta, D, Omega0)
    amp = np.sqrt(2.0 * Q.sf2_of(kind, theta) / Omega0.shape[0])
    ang = np.asarray(V, float) @ om.T + np.asarray(phase, float)[None, :]
    return amp * np.cos(ang), ang, om, amp


def solve_U(kind, X, om, theta, noise, Omega0, phase, W, E=None, route="chol"):
    """U (N, S, P)"""
    X, om = np.asarray(X, float), np.asarray(om, float).reshape(X.shape[0], -1)
    N, D = X.shape
    R, S, P = W.shape
    K = O.kernel_matrix(kind, X, theta, noise)
    solve = Q.solver_chol(K) if route == "chol" else Q.solver_lu(K)
    PhiX = features(kind, theta, D, Omega0, phase, X)[0]
    rhs = om[:, None, :] - np.einsum("nr,rsp->nsp", PhiX, W)
    if E is not None:
        rhs = rhs - np.sqrt(noise + 1e-8) * np.asarray(E, float).reshape(N, S, P)
    return solve(rhs.reshape(N, S * P)).reshape(N, S, P)


def evaluate(kind, X, theta, Omega0, phase, W, U, V, mean_q=None, chunk=128):
    """(F (T, S, P), dF (T, D, S, P)) of a path set given by (W, U); U = None: the prior's paths"""
    X, V = np.asarray(X, float), np.asarray(V, float)
    D = V.shape[1]
    T = V.shape[0]
    R, S, P = W.shape
    Mm, sf2 = Q.mm_matrix(kind, theta, D), Q.sf2_of(kind, theta)
    F, dF = np.zeros((T, S, P)), np.zeros((T, D, S, P))
    for t0 in range(0, T, chunk):
        v = V[t0:t0 + chunk]
        Phi, ang, om, amp = features(kind, theta, D, Omega0, phase, v)
        F[t0:t0 + chunk] = np.einsum("tr,rsp->tsp", Phi, W)
        dPhi = -amp * np.sin(ang)[:, :, None] * om[None, :, :]  # (t, R, D)
        dF[t0:t0 + chunk] = np.einsum("trd,rsp->tdsp", dPhi, W)
        if U is not None and X.shape[0] > 0:
            diff = v[:, None, :] - X[None, :, :]
            md = diff @ Mm
            z = np.einsum("tnd,tnd->tn", md, diff)
            F[t0:t0 + chunk] += np.einsum("tn,nsp->tsp", Q.k_of_z(kind, z, sf2), U)
            dF[t0:t0 + chunk] += np.einsum("tnd,nsp->tdsp", Q.g_of_z(kind, z, sf2)[:, :, None] * md, U)
    if mean_q is not None:
        F = F + np.asarray(mean_q, float).reshape(T, 1, P)
    return F, dF


def reference(kind, X, om, theta, noise, Omega0, phase, W, E, V, mean_q=None, route="chol"):
    U = solve_U(kind, X, om, theta, noise, Omega0, phase, W, E, route)
    return evaluate(kind, X, theta, Omega0, phase, W, U, V, mean_q)


def make_draws(kind, theta, N, D, P, R, S, seed):
    """(Omega0, phase, W (R, S, P), E (N, S, P)) with fixed seeds"""
    Om, ph = spectral_draws(kind, R, freq_dim(kind, theta, D), seed)
    rng = np.random.default_rng(seed + 7919)
    return Om, ph, rng.standard_normal((R, S, P)), rng.standard_normal((N, S, P))


# (kind, N, D, P, Lambda columns) of tests/test_gpu_pathwise.py: parity by kind, the solve's edges, the feature-tile edges' model,
# D = 1 and D = 20, the real size
GPU_SHAPES = [
    (O.SE_ARD, 1100, 6, 1, 0), (O.SE_ARD, 700, 20, 1, 0), (O.SE_ARD, 600, 5, 1, 2), (O.MATERN52, 520, 2, 1, 0), (O.MATERN32, 300, 3, 1, 0),
    (O.EXP, 300, 3, 1, 0), (O.SE_ARD, 1100, 6, 2, 0),
] + [(O.SE_ARD, n, 6, 1, 0) for n in (200, 255, 256, 257, 1024)] + [(O.SE_ARD, 300, 3, 1, 0), (O.SE_ARD, 300, 1, 1, 0), (O.SE_ARD, 4096, 6, 1, 0)]


def routes_disagreement(kind, N, D, P, lam, R=1000, S=8, T=70, seed=5):
    X, om = Q.make_problem(N, D, P, seed)
    th = Q.theta_of(kind, D, lam, seed)
    V = Q.make_points(X, T, seed + 1)
    Om, ph, W, E = make_draws(kind, th, N, D, P, R, S, seed + 2)
    a = reference(kind, X, om, th, NOISE, Om, ph, W, E, V, route="chol")
    b = reference(kind, X, om, th, NOISE, Om, ph, W, E, V, route="lu")
    return [float(np.max(np.abs(p - q))) for p, q in zip(a, b)] + [float(np.max(np.abs(p))) for p in a]


if __name__ == "__main__":
    for shape in GPU_SHAPES:
        print(shape, ["%.2e" % d for d in routes_disagreement(*shape)])
