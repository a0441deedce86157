"""The reference of the expected-hypervolume-improvement tests (tests/test_ehvi_host.py, tests/test_gpu_ehvi.py): never the engine.

ref_ehvi(front, ref, mu1, s1, mu2, s2)   the strip sum of include/gpe_ehvi.h with its four partials in numpy, all candidates and all
                                         strips at once (numpy's pairwise sums, not a wave's order).
mp_ehvi(...)                             the same for ONE candidate in 50-digit arithmetic (mpmath): what ref_ehvi's own error is
                                         measured against; mpf results, so values far below 1e-308 are kept.
mc_hvi(...)                              Monte Carlo: the mean hypervolume improvement of draws (Y1, Y2) and its standard error — no
                                         psi, no strips of the front's own: the area is counted per draw.
hypervolume2(front, ref)                 the area dominated by a prepared front above ref.
pareto_front2(points, ref)               the prepared front of a point set, in plain python (what gpe_ehvi2_front is held against).
Both objectives are maximised; a prepared front is ascending in f1 and descending in f2, all above ref."""
import math

import numpy as np
from scipy.special import erfc

SQRT2, SQRT2PI = math.sqrt(2.0), math.sqrt(2.0 * math.pi)


def pareto_front2(points, ref):
    pts = sorted({(float(a), float(b)) for a, b in np.asarray(points, dtype=float).reshape(-1, 2)
                  if math.isfinite(a) and math.isfinite(b) and a > ref[0] and b > ref[1]})
    keep = [p for p in pts if not any((q[0] >= p[0] and q[1] >= p[1]) and q != p for q in pts)]
    return np.array(keep, dtype=float).reshape(-1, 2)


def is_prepared(front, ref):
    F = np.asarray(front, dtype=float).reshape(-1, 2)
    return bool(np.all(np.isfinite(F)) and np.all(F[:, 0] > ref[0]) and np.all(F[:, 1] > ref[1]) and np.all(np.diff(F[:, 0]) > 0)
                and np.all(np.diff(F[:, 1]) < 0))


def hypervolume2(front, ref):
    F = np.asarray(front, dtype=float).reshape(-1, 2)
    assert is_prepared(F, ref)
    left = np.concatenate([[ref[0]], F[:-1, 0]])
    return float(math.fsum((F[:, 0] - left) * (F[:, 1] - ref[1])))


def _strips(front, ref):
    """l_0 .. l_n (the strips' left ends) and h_0 .. h_n (the front's height above each strip)"""
    F = np.asarray(front, dtype=float).reshape(-1, 2)
    return np.concatenate([[ref[0]], F[:, 0]]), np.concatenate([F[:, 1], [ref[1]]])


def _ev(mu, s, t):
    """(psi, Phi, phi) of the beliefs (mu, s) (M) at the thresholds t (K): M x K each.  s = 0: the limit."""
    mu, s = np.asarray(mu, dtype=float)[:, None], np.asarray(s, dtype=float)[:, None]
    d = mu - t[None, :]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        z = d / np.where(s > 0, s, 1.0)
        a = -np.abs(z)
        phi = np.exp(-0.5 * a * a) / SQRT2PI
        Q = 0.5 * erfc(-a / SQRT2)
        fm = np.maximum(phi + a * Q, 0.0)
        fm = np.where(np.isinf(a), 0.0, fm)
        f = np.where(z < 0, fm, z + fm)
        Phi = np.where(z < 0, Q, 1.0 - Q)
        psi = s * f
    zero = np.broadcast_to(~(s > 0), d.shape)
    psi = np.where(zero, np.maximum(d, 0.0), psi)
    Phi = np.where(zero, (d > 0) * 1.0, Phi)
    phi = np.where(zero, 0.0, phi)
    nan = np.broadcast_to(np.isnan(s) | np.isnan(mu), d.shape)
    return tuple(np.where(nan, np.nan, v) for v in (psi, Phi, phi))


def ref_ehvi(front, ref, mu1, s1, mu2, s2):
    """(ehvi (M), partials (M x 4: d/d mu1, d/d s1, d/d mu2, d/d s2)) for finite beliefs"""
    l, h = _strips(front, ref)
    p1, P1, f1 = _ev(np.atleast_1d(mu1), np.atleast_1d(s1), l)
    p2, P2, f2 = _ev(np.atleast_1d(mu2), np.atleast_1d(s2), h)
    M = p1.shape[0]
    w = np.maximum(p1 - np.concatenate([p1[:, 1:], np.zeros((M, 1))], axis=1), 0.0)  # psi_1(l_i) - psi_1(l_{i+1}), psi_1(inf) = 0
    v = np.maximum(p2 - np.concatenate([np.zeros((M, 1)), p2[:, :-1]], axis=1), 0.0)  # psi_2(h_i) - psi_2(h_{i-1}), psi_2(h_-1) = 0
    with np.errstate(under="ignore"):
        val = np.sum(w * p2, axis=1)
        part = np.stack([np.sum(P1 * v, axis=1), np.sum(f1 * v, axis=1), np.sum(w * P2, axis=1), np.sum(w * f2, axis=1)], axis=1)
    return val, part


def mp_ehvi(front, ref, mu1, s1, mu2, s2, partials=True):
    """one candidate at 50 digits: (ehvi, [d/d mu1, d/d s1, d/d mu2, d/d s2]) as mpf.  The value is the strip sum as written
    (psi_1(l_i) - psi_1(u_i)) psi_2(h_i); the partials in (mu2, s2) are its term-by-term derivatives and those in (mu1, s1) the same
    sum by parts (test_ehvi_host.py holds all four against central differences of the value)."""
    import mpmath as mp

    with mp.workdps(50):
        l, h = _strips(front, ref)
        l, h = [mp.mpf(float(x)) for x in l], [mp.mpf(float(x)) for x in h]
        m1, m2, d1, d2 = (mp.mpf(float(x)) for x in (mu1, mu2, s1, s2))

        def ev(mu, s, t):
            if s == 0:
                d = mu - t
                return (d if d > 0 else mp.mpf(0)), mp.mpf(1 if d > 0 else 0), mp.mpf(0)
            z = (mu - t) / s
            return s * (mp.npdf(z) + z * mp.ncdf(z)), mp.ncdf(z), mp.npdf(z)

        e1 = [ev(m1, d1, t) for t in l] + [(mp.mpf(0),) * 3]
        e2 = [ev(m2, d2, t) for t in h]
        n1 = len(l)
        val = mp.fsum((e1[i][0] - e1[i + 1][0]) * e2[i][0] for i in range(n1))
        if not partials:
            return val, None
        v = [e2[i][0] - (e2[i - 1][0] if i else 0) for i in range(n1)]
        part = [mp.fsum(e1[i][1] * v[i] for i in range(n1)), mp.fsum(e1[i][2] * v[i] for i in range(n1)),
                mp.fsum((e1[i][0] - e1[i + 1][0]) * e2[i][1] for i in range(n1)),
                mp.fsum((e1[i][0] - e1[i + 1][0]) * e2[i][2] for i in range(n1))]
        return val, part


def hvi_points(front, ref, Y):
    """the hypervolume improvement of each point of Y (K x 2) over the front: the part of the box [ref, y] no front point
    dominates, strip by strip — min / max of coordinates only"""
    l, h = _strips(front, ref)
    u = np.concatenate([l[1:], [np.inf]])
    wid = np.clip(np.minimum(Y[:, :1], u[None, :]) - l[None, :], 0.0, None)
    hei = np.clip(Y[:, 1:2] - h[None, :], 0.0, None)
    return np.sum(wid * hei, axis=1)


def mc_hvi(front, ref, mu1, s1, mu2, s2, draws=2_000_000, seed=0, chunk=100_000):
    """(mean, standard error) of the hypervolume improvement over `draws` draws of the two independent Gaussians"""
    rng = np.random.default_rng(seed)
    tot = tot2 = 0.0
    done = 0
    while done < draws:
        k = min(chunk, draws - done)
        Y = np.stack([mu1 + s1 * rng.standard_normal(k), mu2 + s2 * rng.standard_normal(k)], axis=1)
        g = hvi_points(front, ref, Y)
        tot += float(g.sum())
        tot2 += float((g * g).sum())
        done += k
    mean = tot / draws
    return mean, math.sqrt(max(tot2 / draws - mean * mean, 0.0) / draws)
