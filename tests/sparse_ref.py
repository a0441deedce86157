"""numpy / LAPACK references of the sparse pseudo-input GP (include/gpe_sparse.h) — the checker of tests/test_gpu_sparse_gp.py and
of the C++ drop-in's test.  Never the engine.  Two independent routes:

  route_a   the reference's own sequence, src/limbo/experimental/model/spgp.hpp:394-406 (L, V, ep, Lm, bet), :491 (fw, with the
            real (n - m) / 2) and :597-608 (lst, lmst, mu, s2 without the "+ sig" and without the mean functor);
  route_b   the dense definition of the same model (FITC): Q = K_nm K_mm^-1 K_mn by LU, Sigma = Q + diag(c - diag Q) + sig I,
            mu = Q_*n Sigma^-1 y, s2 = c - Q_*n Sigma^-1 Q_n*, nlml = 1/2 log|Sigma| + 1/2 y^T Sigma^-1 y + 1/2 n log 2 pi.

`python -m tests.sparse_ref` prints the disagreement of the two on the shapes the GPU tests use."""
import numpy as np
import scipy.linalg as sla

LD = np.longdouble
ELL6 = np.array([0.3, 0.45, 0.6, 0.75, 0.9, 1.0])  # the length scales of tests/test_gpu_joint_posterior.py's ELL6
LOG_C, LOG_SIG = 0.0, np.log(0.01)                   # c = 1, sig = 0.01


def ells(D):
    return ELL6.copy() if D == 6 else np.linspace(0.3, 1.0, D)


def log_b_of(ell):
    """SPGP's b_d = l_d^-2, in log-space"""
    return -2.0 * np.log(np.asarray(ell, dtype=np.float64))


def make_problem(N, M, D, P, seed, T=400):
    """X uniform in [0, 1]^D, the pseudo-inputs a random subset of X, y = sin(3 X.u) + 0.1 N(0, 1) centred, T test points"""
    rng = np.random.default_rng(seed)
    X = rng.random((N, D))
    Xb = X[rng.permutation(N)[:M]].copy()
    Y = np.stack([np.sin(3.0 * X @ rng.random(D)) + 0.1 * rng.standard_normal(N) for _ in range(P)], axis=1)
    return dict(N=N, M=M, D=D, P=P, X=X, Xb=Xb, y=Y - Y.mean(axis=0), Xt=rng.random((T, D)), log_b=log_b_of(ells(D)), log_c=LOG_C,
                log_sig=LOG_SIG)


def kern(A, B, log_b, log_c):
    """spgp.hpp:612-628: c exp(-1/2 sum_d b_d (a_d - b_d)^2)"""
    sb = np.exp(0.5 * np.asarray(log_b))
    a, b = A * sb, B * sb
    d2 = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * a @ b.T
    return np.exp(log_c) * np.exp(-0.5 * np.maximum(d2, 0.0))


def route_a(X, Xb, y, log_b, log_c, log_sig, jitter, Xt=None):
    n, m = X.shape[0], Xb.shape[0]
    c, sig = np.exp(log_c), np.exp(log_sig)
    L = np.linalg.cholesky(kern(Xb, Xb, log_b, log_c) + jitter * np.eye(m))                 # :394-395
    V = sla.solve_triangular(L, kern(Xb, X, log_b, log_c), lower=True)                      # :396-398
    ep = 1.0 + (c - (V * V).sum(0)) / sig                                                   # :399
    Vs = V / np.sqrt(ep)[None, :]                                                           # :401-402
    ys = y / np.sqrt(ep)[:, None]                                                           # :403
    Lm = np.linalg.cholesky(sig * np.eye(m) + Vs @ Vs.T)                                    # :405
    bet = sla.solve_triangular(Lm, Vs @ ys, lower=True)                                     # :406
    # :491, the sums in extended precision (the matrices above are what the sequence gives in double)
    ysl, betl = ys.astype(LD), bet.astype(LD)
    nlml = (np.log(np.diag(Lm).astype(LD)).sum() + LD(0.5) * (n - m) * LD(log_sig) + ((ysl * ysl).sum(0) - (betl * betl).sum(0)) / (2 * LD(sig))
            + np.log(ep.astype(LD)).sum() / 2 + LD(0.5) * n * np.log(2 * LD(np.pi)))
    out = dict(L=L, Lm=Lm, ep=ep, bet=bet, nlml=nlml.astype(np.float64))
    if Xt is not None:
        lst = sla.solve_triangular(L, kern(Xb, Xt, log_b, log_c), lower=True)               # :597-598
        lmst = sla.solve_triangular(Lm, lst, lower=True)                                    # :599
        out["mu"] = (bet.T @ lmst).T                                                        # :604
        out["s2"] = c - (lst * lst).sum(0) + sig * (lmst * lmst).sum(0)                     # :608
    return out


def route_b(X, Xb, y, log_b, log_c, log_sig, jitter, Xt=None):
    n = X.shape[0]
    c, sig = np.exp(log_c), np.exp(log_sig)
    Kmm = kern(Xb, Xb, log_b, log_c) + jitter * np.eye(Xb.shape[0])
    Kmn = kern(Xb, X, log_b, log_c)
    lu = sla.lu_factor(Kmm)
    Q = Kmn.T @ sla.lu_solve(lu, Kmn)
    Sig = Q + np.diag(c - np.diag(Q)) + sig * np.eye(n)
    Sig = 0.5 * (Sig + Sig.T)
    cf = sla.cho_factor(Sig, lower=True)
    al = sla.cho_solve(cf, y)
    Sl, yl = Sig.astype(LD), y.astype(LD)
    for _ in range(2):  # iterative refinement, the residual in extended precision
        al = al + sla.cho_solve(cf, (yl - Sl @ al.astype(LD)).astype(np.float64))
    nlml = np.log(np.diag(cf[0]).astype(LD)).sum() + LD(0.5) * (yl * al.astype(LD)).sum(0) + LD(0.5) * n * np.log(2 * LD(np.pi))
    out = dict(nlml=nlml.astype(np.float64), ep=(np.diag(Sig) - np.diag(Q)) / sig)
    if Xt is not None:
        Qsn = kern(Xt, Xb, log_b, log_c) @ sla.lu_solve(lu, Kmn)
        out["mu"] = Qsn @ al
        out["s2"] = c - np.einsum("ij,ji->i", Qsn, sla.cho_solve(cf, Qsn.T))
    return out


def disagreement(pr, jitter):
    """max |a - b| of mu and s2, |a - b| / |a| of nlml"""
    a = route_a(pr["X"], pr["Xb"], pr["y"], pr["log_b"], pr["log_c"], pr["log_sig"], jitter, pr["Xt"])
    b = route_b(pr["X"], pr["Xb"], pr["y"], pr["log_b"], pr["log_c"], pr["log_sig"], jitter, pr["Xt"])
    return (float(np.max(np.abs(a["mu"] - b["mu"]))), float(np.max(np.abs(a["s2"] - b["s2"]))),
            float(np.max(np.abs(a["nlml"] - b["nlml"]) / np.abs(a["nlml"]))), a)


if __name__ == "__main__":
    for (N, M, D, P) in [(1300, 40, 3, 1), (1300, 193, 6, 2), (1500, 320, 6, 1), (1500, 256, 20, 1)]:
        for jit in (1e-6, 1e-4):
            pr = make_problem(N, M, D, P, 7)
            dm, ds, dn, a = disagreement(pr, jit)
            Kmm = kern(pr["Xb"], pr["Xb"], pr["log_b"], pr["log_c"]) + jit * np.eye(M)
            print(f"N={N} M={M} D={D} P={P} jitter={jit:g}: cond K_mm = {np.linalg.cond(Kmm):.1e}  |mu a-b| = {dm:.2e}  |s2 a-b| = {ds:.2e}  "
                  f"nlml rel = {dn:.2e} (nlml = {a['nlml']})")
