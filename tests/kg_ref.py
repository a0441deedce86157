"""The reference of the knowledge-gradient tests (tests/test_kg_host.py, tests/test_gpu_kg.py): never the engine, and deliberately
not the engine's construction.

ref_h(a, b)     h = E[max_i (a_i + b_i Z)] - max_i a_i by the SORTED STACK algorithm of Frazier, Powell, Dayanik (2009), Algorithm 1:
                sort by slope, drop all but the largest a of equal slopes, push the lines one by one and pop those the new line
                covers; then sum (b_next - b_cur) f(-|c|) over the breakpoints c that are left.  The engine builds a successor
                chain with no sort and no stack (include/gpe_kg.h).
mp_h(a, b)      the same quantity in 50-digit arithmetic (mpmath) for A <= 64: what ref_h's own error is measured against.
ref_kg(...)     the quantity of gpe_kg_batch on a covariance Sig and means mu formed in numpy."""
import math

import numpy as np

EPS = np.finfo(float).eps
SQRT2, SQRT2PI = math.sqrt(2.0), math.sqrt(2.0 * math.pi)


def f_neg(z):
    """f(-|z|) = phi(z) - |z| Phi(-|z|) >= 0 in double precision (loses about z^2 ulps to cancellation at large |z|)"""
    t = -abs(z)
    if math.isinf(t):
        return 0.0
    return max(math.exp(-0.5 * t * t) / SQRT2PI + t * 0.5 * math.erfc(-t / SQRT2), 0.0)


def _stack(a, b, div, inf):
    """the lines (sorted, deduplicated) that form the upper envelope and the breakpoints between neighbours"""
    order = sorted(range(len(a)), key=lambda i: (b[i], a[i]))
    keep = [i for k, i in enumerate(order) if k + 1 == len(order) or b[order[k + 1]] != b[i]]  # the largest a of equal slopes
    st, c = [keep[0]], [-inf]  # c[k]: where st[k] takes over from st[k - 1]
    for i in keep[1:]:
        while True:
            j = st[-1]
            z = div(a[j] - a[i], b[i] - b[j])
            if len(st) > 1 and z <= c[-1]:
                st.pop()
                c.pop()
                continue
            break
        st.append(i)
        c.append(z)
    return st, c


def ref_h(a, b):
    a, b = [float(x) for x in np.asarray(a).ravel()], [float(x) + 0.0 for x in np.asarray(b).ravel()]  # (+ 0.0: -0.0 sorts as 0.0)
    st, c = _stack(a, b, lambda x, y: x / y, math.inf)
    return math.fsum((b[st[k]] - b[st[k - 1]]) * f_neg(c[k]) for k in range(1, len(st)))


def ref_nseg(a, b):
    a, b = [float(x) for x in np.asarray(a).ravel()], [float(x) + 0.0 for x in np.asarray(b).ravel()]
    return len(_stack(a, b, lambda x, y: x / y, math.inf)[0]) - 1


def mp_h(a, b):
    import mpmath as mp

    assert len(a) <= 64
    with mp.workdps(50):
        aa, bb = [mp.mpf(float(x)) for x in a], [mp.mpf(float(x)) for x in b]
        st, c = _stack(aa, bb, lambda x, y: x / y, mp.inf)
        tot = mp.mpf(0)
        for k in range(1, len(st)):
            t = -abs(c[k])
            tot += (bb[st[k]] - bb[st[k - 1]]) * (mp.npdf(t) + t * mp.ncdf(t))
        return tot  # (an mpf: values below 1e-308 are kept)


def ref_kg(Sig, mu, A_idx, C_idx, lam, with_self):
    """kg[m] for the candidates C_idx over the alternatives A_idx of a joint belief N(mu, Sig); lam: the observation noise"""
    A_idx, C_idx = np.asarray(A_idx), np.asarray(C_idx)
    out = np.zeros(len(C_idx))
    for k, m in enumerate(C_idx):
        out[k] = ref_kg_column(mu[A_idx], Sig[A_idx, m], Sig[m, m], mu[m], lam, with_self)
    return out


def ref_kg_column(a, c, s, mu_m, lam, with_self):
    d = s + lam
    if not (d > EPS) or not math.isfinite(d):
        return 0.0
    b = np.asarray(c) / math.sqrt(d)
    a = np.asarray(a)
    if with_self:
        a, b = np.append(a, mu_m), np.append(b, s / math.sqrt(d))
    return ref_h(a, b)
