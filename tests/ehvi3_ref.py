"""The reference of the three-objective expected-hypervolume-improvement tests (tests/test_ehvi3_host.py, tests/test_gpu_ehvi3.py):
never the engine.

pareto_front3(points, ref)     the prepared front of a point set in plain quadratic python (what gpe_ehvi3_front is held against).
boxes3(front, ref, c)          the table of include/gpe_ehvi3.h for the height axis c: the sweep with a python list as staircase.
ref_ehvi3(front, ref, mu, s)   the three box sums with the six partials in numpy, all candidates and all boxes at once (numpy's
                               pairwise sums, not a wave's order).
height_grid(front, ref, c)     the height field by brute force on the grid of the front's coordinates: no sweep, no boxes.
mp_ehvi3(...)                  ONE candidate in 50-digit arithmetic (mpmath) over the cells of that grid — an independent
                               construction: what ref_ehvi3's own error is measured against; mpf results, so values far below
                               1e-308 are kept.
mc_hvi3(...)                   Monte Carlo: the mean hypervolume improvement of draws (Y1, Y2, Y3) and its standard error — no psi.
hypervolume3(front, ref)       the dominated volume by inclusion of grid cells.
All objectives are maximised; a prepared front is descending in f3 (ties ascending in f1, then f2), all above ref."""
import bisect
import math

import numpy as np

from tests.ehvi_ref import _ev


def dominates(q, p):
    return all(a >= b for a, b in zip(q, p)) and tuple(q) != tuple(p)


def pareto_front3(points, ref):
    pts = {(float(a), float(b), float(c)) for a, b, c in np.asarray(points, dtype=float).reshape(-1, 3)
           if all(math.isfinite(v) for v in (a, b, c)) and a > ref[0] and b > ref[1] and c > ref[2]}
    keep = [p for p in pts if not any(dominates(q, p) for q in pts)]
    keep.sort(key=lambda p: (-p[2], p[0], p[1]))
    return np.array(keep, dtype=float).reshape(-1, 3)


def is_prepared3(front, ref):
    F = np.asarray(front, dtype=float).reshape(-1, 3)
    if not (np.all(np.isfinite(F)) and np.all(F > np.asarray(ref, dtype=float)[None, :])):
        return False
    rows = [tuple(p) for p in F]
    if any(dominates(q, p) for p in rows for q in rows) or len(set(rows)) != len(rows):
        return False
    return rows == sorted(rows, key=lambda p: (-p[2], p[0], p[1]))


def plane_axes(c):
    return (1 if c == 0 else 0), (1 if c == 2 else 2)


def boxes3(front, ref, c):
    """rows {l_a, u_a, l_b, u_b, h}: sweep descending in f_c (stable), the staircase of the (a, b) plane as a sorted list"""
    F = np.asarray(front, dtype=float).reshape(-1, 3)
    a, b = plane_axes(c)
    order = sorted(range(len(F)), key=lambda i: -F[i, c])
    stair, rows = [], []  # stair: (a, b), ascending in a, descending in b

    def row(la, ua, lb, ub, h):
        if la < ua and lb < ub:
            rows.append((la, ua, lb, ub, h))

    for i in order:
        qa, qb, qc = F[i, a], F[i, b], F[i, c]
        hi = bisect.bisect_right([p[0] for p in stair], qa)
        lo = hi
        while lo > 0 and stair[lo - 1][1] <= qb:
            lo -= 1
        left = stair[lo - 1][0] if lo > 0 else ref[a]
        for j in range(lo, hi):
            row(left, stair[j][0], stair[j][1], qb, qc)
            left = stair[j][0]
        row(left, qa, stair[hi][1] if hi < len(stair) else ref[b], qb, qc)
        stair[lo:hi] = [(qa, qb)]
    left = ref[a]
    for pa, pb in stair:
        row(left, pa, pb, math.inf, ref[c])
        left = pa
    row(left, math.inf, ref[b], math.inf, ref[c])
    return np.array(rows, dtype=float).reshape(-1, 5)


def box_sums(B, mu_a, s_a, mu_b, s_b, mu_c, s_c):
    """(value, d/d mu_c, d/d s_c), M each, over the table B"""
    pal, pau = _ev(mu_a, s_a, B[:, 0])[0], _ev(mu_a, s_a, B[:, 1])[0]
    pbl, pbu = _ev(mu_b, s_b, B[:, 2])[0], _ev(mu_b, s_b, B[:, 3])[0]
    pc, Pc, fc = _ev(mu_c, s_c, B[:, 4])
    with np.errstate(under="ignore"):
        w = np.maximum(pal - pau, 0.0) * np.maximum(pbl - pbu, 0.0)
        return np.sum(w * pc, axis=1), np.sum(w * Pc, axis=1), np.sum(w * fc, axis=1)


def ref_ehvi3(front, ref, mu, s, value_axis=2):
    """(ehvi (M), partials (M x 6: d/d mu1, d/d s1, d/d mu2, d/d s2, d/d mu3, d/d s3)) for finite beliefs mu, s (M x 3); the value
    from the table of height axis value_axis"""
    mu, s = np.asarray(mu, dtype=float).reshape(-1, 3), np.asarray(s, dtype=float).reshape(-1, 3)
    part = np.zeros((mu.shape[0], 6))
    val = None
    for c in range(3):
        a, b = plane_axes(c)
        v, part[:, 2 * c], part[:, 2 * c + 1] = box_sums(boxes3(front, ref, c), mu[:, a], s[:, a], mu[:, b], s[:, b], mu[:, c], s[:, c])
        if c == value_axis:
            val = v
    return val, part


def height_grid(front, ref, c):
    """(xa, xb, H): the sorted distinct coordinates of axes a < b (ref first) and H[i, j], the largest f_c among the front points
    with f_a > xa[i] and f_b > xb[j], ref[c] if there is none: the height over the cell [xa[i], xa[i+1]) x [xb[j], xb[j+1])"""
    F = np.asarray(front, dtype=float).reshape(-1, 3)
    a, b = plane_axes(c)
    xa = np.array(sorted({float(ref[a])} | set(F[:, a].tolist())))
    xb = np.array(sorted({float(ref[b])} | set(F[:, b].tolist())))
    H = np.full((len(xa), len(xb)), float(ref[c]))
    for p in F:
        H = np.where((p[a] > xa)[:, None] & (p[b] > xb)[None, :], np.maximum(H, p[c]), H)
    return xa, xb, H


def hypervolume3(front, ref):
    xa, xb, H = height_grid(front, ref, 2)
    if len(xa) < 2 or len(xb) < 2:
        return 0.0
    vol = np.diff(xa)[:, None] * np.diff(xb)[None, :] * (H[:-1, :-1] - ref[2])
    return float(math.fsum(vol.ravel()))


def mp_ehvi3(front, ref, mu, s, partials=True, dps=50):
    """one candidate at `dps` digits: (ehvi, [d/d mu1, d/d s1, d/d mu2, d/d s2, d/d mu3, d/d s3]) as mpf.  The value is the sum over
    the cells of the grid the front's coordinates span: (psi_1(x_i) - psi_1(x_i+1)) (psi_2(y_j) - psi_2(y_j+1)) psi_3(H_ij), the
    cells above H_ij in the third axis summed in closed form (they telescope to psi_3(H_ij)).  The partials are the term-by-term
    derivatives of that one sum: Phi and phi in psi's place, differences included; Phi(x) - Phi(x') is formed from the upper tails
    where both arguments are positive, so that it keeps its digits."""
    import mpmath as mp

    with mp.workdps(dps):
        xa, xb, H = height_grid(front, ref, 2)
        m = [v if isinstance(v, mp.mpf) else mp.mpf(float(v)) for v in mu]  # (mpf inputs are taken as they are: the central differences)
        d = [v if isinstance(v, mp.mpf) else mp.mpf(float(v)) for v in s]
        assert len(m) == 3 and len(d) == 3
        zero = mp.mpf(0)

        def ev(k, t):  # (psi, Phi, 1 - Phi, phi) of objective k at t
            if t is None:
                return zero, zero, mp.mpf(1), zero
            t = mp.mpf(float(t))
            if d[k] == 0:
                x = m[k] - t
                return (x if x > 0 else zero), mp.mpf(1 if x > 0 else 0), mp.mpf(0 if x > 0 else 1), zero
            z = (m[k] - t) / d[k]
            return d[k] * (mp.npdf(z) + z * mp.ncdf(z)), mp.ncdf(z), mp.ncdf(-z), mp.npdf(z)

        def diffs(k, xs):  # per cell: psi(l) - psi(u), Phi(l) - Phi(u), phi(l) - phi(u); the last cell's u is +inf
            e = [ev(k, t) for t in xs] + [ev(k, None)]
            return [(e[i][0] - e[i + 1][0], (e[i + 1][2] - e[i][2]) if e[i + 1][1] > 0.5 else (e[i][1] - e[i + 1][1]), e[i][3] - e[i + 1][3])
                    for i in range(len(xs))]

        A, B = diffs(0, xa), diffs(1, xb)
        hs = {float(h): ev(2, h) for h in np.unique(H)}
        Ec = [[hs[float(H[i, j])] for j in range(len(xb))] for i in range(len(xa))]
        cells = [(i, j) for i in range(len(xa)) for j in range(len(xb))]
        val = mp.fsum(A[i][0] * B[j][0] * Ec[i][j][0] for i, j in cells)
        if not partials:
            return val, None
        part = [mp.fsum(A[i][1] * B[j][0] * Ec[i][j][0] for i, j in cells), mp.fsum(A[i][2] * B[j][0] * Ec[i][j][0] for i, j in cells),
                mp.fsum(A[i][0] * B[j][1] * Ec[i][j][0] for i, j in cells), mp.fsum(A[i][0] * B[j][2] * Ec[i][j][0] for i, j in cells),
                mp.fsum(A[i][0] * B[j][0] * Ec[i][j][1] for i, j in cells), mp.fsum(A[i][0] * B[j][0] * Ec[i][j][3] for i, j in cells)]
        return val, part


def hvi_points3(front, ref, Y):
    """the hypervolume improvement of each point of Y (K x 3) over the front: the part of the box [ref, y] no front point dominates,
    box by box of the table of height axis 3 — min / max of coordinates only"""
    B = boxes3(front, ref, 2)
    wa = np.clip(np.minimum(Y[:, 0:1], B[None, :, 1]) - B[None, :, 0], 0.0, None)
    wb = np.clip(np.minimum(Y[:, 1:2], B[None, :, 3]) - B[None, :, 2], 0.0, None)
    return np.sum(wa * wb * np.clip(Y[:, 2:3] - B[None, :, 4], 0.0, None), axis=1)


def mc_hvi3(front, ref, mu, s, draws=1_000_000, seed=0, chunk=100_000):
    """(mean, standard error) of the hypervolume improvement over `draws` draws of the three independent Gaussians"""
    rng = np.random.default_rng(seed)
    mu, s = np.asarray(mu, dtype=float).reshape(1, 3), np.asarray(s, dtype=float).reshape(1, 3)
    tot = tot2 = 0.0
    done = 0
    while done < draws:
        k = min(chunk, draws - done)
        g = hvi_points3(front, ref, mu + s * rng.standard_normal((k, 3)))
        tot += float(g.sum())
        tot2 += float((g * g).sum())
        done += k
    mean = tot / draws
    return mean, math.sqrt(max(tot2 / draws - mean * mean, 0.0) / draws)
