"""The reference of the noisy-expected-improvement tests (tests/test_nei_host.py, tests/test_gpu_nei.py): never the engine.

ref_lognei(fplus, xi, cmean, csd)        include/gpe_nei.h's kernel in numpy / scipy for all candidates at once: (lognei (M), terms
                                         (S, M)); cmean is (S, M), csd (M) standard deviations.  log h follows tests/cei_ref.py's forms.
term_partials(fplus, xi, cmean, csd)     (d term_s / d cmean_s, d term_s / d sd), (S, M) each: what pushes a bar on the inputs through
                                         to first order.
mp_lognei(fplus, xi, cmean_col, sd)      the same for ONE candidate with sd > 0 in 50-digit arithmetic (mpmath), from the definition
                                         phi + z Phi itself (below z = -1000 from Mills' ratio's asymptotic series): what ref_lognei's own error is
                                         measured against.  (The difference cancels about log10(z^2) digits: the working precision
                                         is raised by that many.)
ref_pipeline(...)                        the whole of gpe_lognei_batch from a LAPACK factor of the model: the baseline's covariance, its
                                         factor, the draws and their maxima, and per candidate c, u = L_b^-1 c, cmean, cvar, lognei.
mp_augmented(...)                        the posterior at the candidates of the model of order N + B that also holds the fantasies
                                         (Xb, F[:, s]) observed with noise variance `jitter`, in mpmath: what (cmean, cvar) must equal.
err(got, truth)                          tests/cei_ref.py's measure |got - truth| / max(1, |truth|)."""
import math

import numpy as np
import scipy.linalg as sla

from oracle import np_oracle as O
from tests.cei_ref import _log_h, err  # noqa: F401  (err is part of this module's interface)

EPS = np.finfo(float).eps
MAX_BASELINE, MAX_SAMPLES = 1024, 1024


def _terms(fplus, xi, cmean, csd):
    fplus = np.asarray(fplus, dtype=float).reshape(-1)
    S = fplus.shape[0]
    cmean = np.asarray(cmean, dtype=float).reshape(S, -1)
    csd = np.asarray(csd, dtype=float).reshape(-1)
    with np.errstate(all="ignore"):
        d = cmean - fplus[:, None] - xi
        pos = csd > 0
        sp = np.where(pos, csd, 1.0)[None, :]
        z = d / sp
        fin = np.isfinite(z)
        lh, rP, rp = _log_h(np.where(fin, z, 0.0))
        t = np.log(sp) + lh
        t = np.where(z == np.inf, np.inf, np.where(z == -np.inf, -np.inf, t))
        rP = np.where(fin, rP, 0.0)
        rp = np.where(fin, rp, 0.0)
        t0 = np.where(d > 0, np.log(np.where(d > 0, d, 1.0)), -np.inf)  # sd = 0: the improvement itself, or none
        t = np.where(pos[None, :], t, t0)
        bad = np.isnan(d) | np.isnan(csd)[None, :]
        t = np.where(bad, np.nan, t)
    return t, rP / sp, rp / sp


def ref_lognei(fplus, xi, cmean, csd):
    t, _, _ = _terms(fplus, xi, cmean, csd)
    S = t.shape[0]
    with np.errstate(all="ignore"):
        top = t.max(axis=0)
        fin = np.isfinite(top)
        e = np.exp(t - np.where(fin, top, 0.0)[None, :])
        val = np.where(fin, top + np.log(e.sum(axis=0)) - math.log(S), top)
    bad = np.isnan(t).any(axis=0)
    val = np.where(bad, np.nan, val)
    t = np.where(bad[None, :], np.nan, t)
    return val, t


def term_partials(fplus, xi, cmean, csd):
    _, dm, ds = _terms(fplus, xi, cmean, csd)
    return dm, ds


def mp_lognei(fplus, xi, cmean_col, sd):
    """one candidate, sd > 0, finite inputs: (lognei, [terms]) as mpf"""
    import mpmath as mp

    fplus = [float(v) for v in np.asarray(fplus, dtype=float).reshape(-1)]
    cm = [float(v) for v in np.asarray(cmean_col, dtype=float).reshape(-1)]
    S = len(fplus)
    zmax = max([1.0] + [abs((cm[s] - fplus[s] - xi) / float(sd)) for s in range(S)])
    with mp.workdps(50 + int(2 * math.log10(zmax)) + 15):
        s_ = mp.mpf(float(sd))
        terms = []
        for k in range(S):
            z = (mp.mpf(cm[k]) - mp.mpf(fplus[k]) - mp.mpf(float(xi))) / s_
            if z < -1000:  # 1 - x R(x) = sum_k (-1)^(k+1) (2k - 1)!! / x^(2k): alternating, the error below the first term left out
                x2, q, ser = z * z, mp.mpf(1), mp.mpf(0)
                for j in range(1, 40):
                    q = q * (2 * j - 1) / x2
                    ser += q if j % 2 else -q
                lh = -x2 / 2 - mp.log(2 * mp.pi) / 2 + mp.log(ser)
            else:
                lh = mp.log(mp.npdf(z) + z * mp.ncdf(z))
            terms.append(mp.log(s_) + lh)
        top = max(terms)
        val = top + mp.log(mp.fsum(mp.exp(t - top) for t in terms)) - mp.log(S)
        return val, terms


def ref_pipeline(kind, th, noise, X, om, out, Xb, mean_b, jitter, Z, xi, Xc, mean_add, L=None, alpha=None):
    """include/gpe_nei.h's quantities for the model (X, om) — from the factor L and alpha given, else from LAPACK's"""
    if L is None:
        _, L, alpha = O.gp_fit(kind, X, om, th, noise)
    Xb, Xc = np.asarray(Xb, dtype=float), np.asarray(Xc, dtype=float)
    B, M = Xb.shape[0], Xc.shape[0]
    Z = np.asarray(Z, dtype=float).reshape(B, -1)
    S = Z.shape[1]
    al = np.asarray(alpha, dtype=float).reshape(X.shape[0], -1)[:, out]
    Kb = O.kernel_cross(kind, X, Xb, th)
    Zb = sla.solve_triangular(L, Kb, lower=True)
    mu_b = Kb.T @ al + (0.0 if mean_b is None else np.asarray(mean_b, dtype=float))
    Sig = O.kernel_cross(kind, Xb, Xb, th) - Zb.T @ Zb + jitter * np.eye(B)
    Sig = 0.5 * (Sig + Sig.T)
    Lb = sla.cholesky(Sig, lower=True)
    F = mu_b[:, None] + Lb @ Z
    fplus = F.max(axis=0)
    Kc = O.kernel_cross(kind, X, Xc, th)
    Zc = sla.solve_triangular(L, Kc, lower=True)
    mu = Kc.T @ al + (0.0 if mean_add is None else np.asarray(mean_add, dtype=float))
    kvv = np.array([O.kernel_cross(kind, Xc[m:m + 1], Xc[m:m + 1], th)[0, 0] for m in range(M)])
    var = kvv - np.sum(Zc * Zc, axis=0)
    Cx = O.kernel_cross(kind, Xb, Xc, th) - Zb.T @ Zc
    U = sla.solve_triangular(Lb, Cx, lower=True)
    cmean = mu[None, :] + Z.T @ U
    cvar = var - np.sum(U * U, axis=0)
    sd = np.sqrt(np.where(cvar > EPS, cvar, 0.0))
    lognei, terms = ref_lognei(fplus, xi, cmean, sd)
    return dict(fplus=fplus, mu=mu, var=var, cvar=cvar, cmean=cmean, sd=sd, lognei=lognei, terms=terms, F=F, Sig=Sig, cond=np.linalg.cond(Sig))


def mp_augmented(kind, th, noise, X, om_col, Xb, F, jitter, Xc, dps=50):
    """(mean (S, M), var (M)) at Xc of the zero-mean model with samples [X; Xb], observations [om_col; F[:, s]] and noise variances
    `noise + 1e-8` on X (kernel.hpp:83) and `jitter` on Xb, in mpmath.  The kernel values are numpy's, taken as exact."""
    import mpmath as mp

    X, Xb, Xc = (np.asarray(a, dtype=float) for a in (X, Xb, Xc))
    N, B, M = X.shape[0], Xb.shape[0], Xc.shape[0]
    Xa = np.vstack([X, Xb])
    K = O.kernel_cross(kind, Xa, Xa, th)
    K = np.tril(K) + np.tril(K, -1).T
    Ks = O.kernel_cross(kind, Xa, Xc, th)
    kvv = [O.kernel_cross(kind, Xc[m:m + 1], Xc[m:m + 1], th)[0, 0] for m in range(M)]
    with mp.workdps(dps):
        A = mp.matrix(K.tolist())
        for i in range(N):
            A[i, i] += mp.mpf(float(noise)) + mp.mpf("1e-8")
        for i in range(B):
            A[N + i, N + i] += mp.mpf(float(jitter))
        Y = mp.matrix(np.vstack([np.tile(np.asarray(om_col, dtype=float).reshape(N, 1), (1, F.shape[1])), F]).tolist())
        Ai = A ** -1
        R = mp.matrix(Ks.tolist())
        W = Ai * R  # (N + B) x M
        mean = Y.T * W  # S x M
        var = [mp.mpf(float(kvv[m])) - mp.fsum(R[i, m] * W[i, m] for i in range(N + B)) for m in range(M)]
        return (np.array([[float(mean[s, m]) for m in range(M)] for s in range(F.shape[1])]), np.array([float(v) for v in var]))
