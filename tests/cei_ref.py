"""The reference of the constrained-expected-improvement tests (tests/test_cei_host.py, tests/test_gpu_cei.py): never the engine.

ref_logcei(with_ei, f_best, xi, thr, mu0, s0, mu_c, s_c)   include/gpe_cei.h in numpy / scipy for all candidates at once: (logcei (M),
                                                           terms (M, 1 + C), partials (M, 2 + 2 C)).
mp_logcei(...)                                             the same for ONE candidate in 50-digit arithmetic (mpmath), from the
                                                           definition phi + z Phi itself: what ref_logcei's own error is measured
                                                           against.  (The difference cancels about log10(z^2) digits: the working
                                                           precision is raised by that many.)
err(got, truth)                                            |got - truth| / max(1, |truth|): the measure of every comparison, logs
                                                           and partials alike; equal infinities count as 0.
ref_logcei uses scipy's log_ndtr for log Phi and, below CROSSOVER, the continued fraction T(x) = 1 / (x + 2 / (x + 3 / ...)) to a depth
far beyond need (REF_DEPTH); above it the direct forms."""
import math

import numpy as np
from scipy.special import erfc, log_ndtr

SQRT2, SQRT2PI, LOG_SQRT2PI = math.sqrt(2.0), math.sqrt(2.0 * math.pi), 0.5 * math.log(2.0 * math.pi)
CROSSOVER = 3.0  # the kernel's (limbo_amd/csrc/logh.h: LOGH_XC); the tests probe both sides of it
REF_DEPTH = 400
MAX_CONSTRAINTS = 16


def err(got, truth):
    got, truth = np.asarray(got, dtype=float), np.asarray(truth, dtype=float)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - truth) / np.maximum(1.0, np.abs(truth))
    same = (got == truth) | (np.isnan(got) & np.isnan(truth))
    return np.where(same, 0.0, np.where(np.isnan(e), np.inf, e))


def _T(x, depth=REF_DEPTH):
    """T(x) = 1 / R(x) - x for x > 0 by the continued fraction, bottom-up"""
    t = x.copy()
    for k in range(depth, 1, -1):
        t = x + k / t
    return 1.0 / t


def _log_h(z):
    """(log h, Phi / h, phi / h) of h(z) = phi(z) + z Phi(z), elementwise; finite z"""
    z = np.asarray(z, dtype=float)
    lo = z < -CROSSOVER
    x = np.where(lo, -z, CROSSOVER)
    with np.errstate(all="ignore"):
        T = _T(x)
        rinv = x + T  # 1 / R(x)
        lh_lo = -0.5 * x * x - LOG_SQRT2PI - np.log(rinv) + np.log(T)
        a = np.abs(np.where(lo, 0.0, z))
        phi = np.exp(-0.5 * a * a) / SQRT2PI
        Q = 0.5 * erfc(a / SQRT2)
        fm = phi - a * Q
        zz = np.where(lo, 0.0, z)
        h = np.where(zz < 0, fm, zz + fm)
        Phi = np.where(zz < 0, Q, 1.0 - Q)
        lh = np.where(lo, lh_lo, np.log(h))
        r_Phi = np.where(lo, 1.0 / T, Phi / h)
        r_phi = np.where(lo, rinv / T, phi / h)
    return lh, r_Phi, r_phi


def _log_Phi(u):
    """(log Phi(u), lambda(u) = phi / Phi)"""
    u = np.asarray(u, dtype=float)
    lo = u < -CROSSOVER
    x = np.where(lo, -u, CROSSOVER)
    with np.errstate(all="ignore"):
        lam_lo = x + _T(x)
        lP = log_ndtr(u)
        uu = np.where(lo, 0.0, u)
        lam = np.where(lo, lam_lo, np.exp(-0.5 * uu * uu - lP) / SQRT2PI)
    return lP, lam


def ref_logcei(with_ei, f_best, xi, thr, mu0, s0, mu_c, s_c):
    thr = np.asarray(thr, dtype=float).reshape(-1)
    C = thr.shape[0]
    mu0, s0 = np.atleast_1d(np.asarray(mu0, dtype=float)), np.atleast_1d(np.asarray(s0, dtype=float))
    M = mu0.shape[0]
    mu_c, s_c = np.asarray(mu_c, dtype=float).reshape(M, C), np.asarray(s_c, dtype=float).reshape(M, C)
    terms, part = np.zeros((M, 1 + C)), np.zeros((M, 2 + 2 * C))
    with np.errstate(all="ignore"):
        if with_ei:
            d = mu0 - f_best - xi
            pos = s0 > 0
            lh, rP, rp = _log_h(np.where(pos, d / np.where(pos, s0, 1.0), 0.0))
            sp = np.where(pos, s0, 1.0)
            terms[:, 0] = np.where(pos, np.log(sp) + lh, np.where(d > 0, np.log(np.where(d > 0, d, 1.0)), -np.inf))
            part[:, 0] = np.where(pos, rP / sp, np.where(d > 0, 1.0 / np.where(d > 0, d, 1.0), 0.0))
            part[:, 1] = np.where(pos, rp / sp, 0.0)
            bad = np.isnan(d) | np.isnan(s0)
            terms[bad, 0] = np.nan
            part[bad, :2] = np.nan
        for k in range(C):
            dk = mu_c[:, k] - thr[k]
            pos = s_c[:, k] > 0
            sp = np.where(pos, s_c[:, k], 1.0)
            u = np.where(pos, dk / sp, 0.0)
            lP, lam = _log_Phi(u)
            terms[:, 1 + k] = np.where(pos, lP, np.where(dk >= 0, 0.0, -np.inf))
            part[:, 2 + k] = np.where(pos, lam / sp, 0.0)
            part[:, 2 + C + k] = np.where(pos, -u * lam / sp, 0.0)
            bad = np.isnan(dk) | np.isnan(s_c[:, k])
            terms[bad, 1 + k] = np.nan
            part[bad, 2 + k] = part[bad, 2 + C + k] = np.nan
        val = terms.sum(axis=1)
    return val, terms, part


def mp_logcei(with_ei, f_best, xi, thr, mu0, s0, mu_c, s_c):
    """one candidate, s > 0 throughout: (logcei, [terms], [partials]) as mpf"""
    import mpmath as mp

    thr = [float(t) for t in np.asarray(thr, dtype=float).reshape(-1)]
    mu_c, s_c = np.asarray(mu_c, dtype=float).reshape(-1), np.asarray(s_c, dtype=float).reshape(-1)
    C = len(thr)
    zmax = 1.0
    if with_ei:
        zmax = max(zmax, abs((float(mu0) - f_best - xi) / float(s0)))
    for k in range(C):
        zmax = max(zmax, abs((mu_c[k] - thr[k]) / s_c[k]))
    with mp.workdps(50 + int(2 * math.log10(zmax)) + 5):
        terms, pm, ps = [mp.mpf(0)], [mp.mpf(0)], [mp.mpf(0)]
        if with_ei:
            m, s = mp.mpf(float(mu0)), mp.mpf(float(s0))
            z = (m - mp.mpf(float(f_best)) - mp.mpf(float(xi))) / s
            h = mp.npdf(z) + z * mp.ncdf(z)
            terms, pm, ps = [mp.log(s) + mp.log(h)], [mp.ncdf(z) / (s * h)], [mp.npdf(z) / (s * h)]
        for k in range(C):
            s = mp.mpf(float(s_c[k]))
            u = (mp.mpf(float(mu_c[k])) - mp.mpf(thr[k])) / s
            lam = mp.npdf(u) / mp.ncdf(u)
            terms.append(mp.log(mp.ncdf(u)))
            pm.append(lam / s)
            ps.append(-u * lam / s)
        return mp.fsum(terms), terms, [pm[0], ps[0]] + pm[1:] + ps[1:]
