"""Inputs of the three-objective expected-hypervolume-improvement tests: fronts on the unit sphere's positive octant and on a
coarse lattice (ties in every coordinate), the reference point REF3 below them, and beliefs that put the value anywhere from order one
down to 1e-280."""
import json
from pathlib import Path

import numpy as np

from tests import ehvi3_ref as R

REF3 = (-0.1, -0.2, -0.15)
GOLDEN = Path(__file__).resolve().parent / "golden" / "ehvi3d_reference.json"


def sphere_front(n, rng):
    """n points of f1^2 + f2^2 + f3^2 = 1 with coordinates in (0.02, 1): none dominates another; prepared (descending in f3)"""
    P = np.zeros((0, 3))
    while len(P) < n:
        Q = np.abs(rng.standard_normal((2 * n + 8, 3)))
        Q /= np.linalg.norm(Q, axis=1, keepdims=True)
        P = np.vstack([P, Q[np.all(Q > 0.02, axis=1)]])
    P = P[:n]
    F = P[np.lexsort((P[:, 1], P[:, 0], -P[:, 2]))]
    assert len(np.unique(F[:, 2])) == n
    return F.reshape(n, 3)


def lattice_front(k, q, rng):
    """the front of k random points of the lattice {1/q, .., 1}^3 near the plane i + j + l = 3 q / 2: ties in every coordinate, fewer
    than 2n + 1 boxes"""
    ij = rng.integers(1, q + 1, size=(k, 2))
    l = (3 * q) // 2 - ij.sum(axis=1) + rng.integers(0, 2, size=k)
    P = np.column_stack([ij, l])[(l >= 1) & (l <= q)]
    return R.pareto_front3(P / float(q), REF3)


def lattice_front_with_boxes(rows, axis=2):
    """a lattice front whose table of height axis `axis` has exactly `rows` rows (the first found in a fixed search order)"""
    for seed in range(400):
        F = lattice_front(100 + 9 * (seed % 37), 12 + seed % 7, np.random.default_rng(7000 + seed))
        if len(R.boxes3(F, REF3, axis)) == rows:
            return F
    raise AssertionError(f"no lattice front with {rows} boxes in the search range")


def near_beliefs(F, M, rng, ref=REF3):
    """beliefs within 6 standard deviations of the front: mu_k = t_k + u_k s_k with t a front point (ref if there is none), half of
    the candidates with every u_k in (-0.5, 3) — near or beyond the front — the others with u_k in (-6, 3); log s ~ N(-1.2, 0.6^2)"""
    F = np.asarray(F, dtype=float).reshape(-1, 3)
    t = F[rng.integers(0, len(F), size=M)] if len(F) else np.tile(np.asarray(ref, dtype=float), (M, 1))
    s = np.exp(-1.2 + 0.6 * rng.standard_normal((M, 3)))
    near = rng.uniform(size=(M, 1)) < 0.5
    u = np.where(near, rng.uniform(-0.5, 3.0, size=(M, 3)), rng.uniform(-6.0, 3.0, size=(M, 3)))
    return t + u * s, s


def random_beliefs(M, rng):
    """mu ~ N(0.5, 0.6^2), log s ~ N(-1.5, 1.2^2), each objective: (mu, s), M x 3 each"""
    return 0.5 + 0.6 * rng.standard_normal((M, 3)), np.exp(-1.5 + 1.2 * rng.standard_normal((M, 3)))


def golden_cases():
    """tests/golden/ehvi3d_reference.json: name, n, front, ref, mu, s, `sliceupdate` and `8term` (the reference implementation's
    ehvi3d_sliceupdate and ehvi3d_8term in double precision) and `exact` (the 50-digit value rounded to double)"""
    return json.loads(GOLDEN.read_text())["cases"]


def tail_cases():
    """(name, front, mu, s): candidates deep inside the dominated region — the value falls to 1e-280 as the distance of mu below the
    front grows to 35 standard deviations in one objective, or about 20 in all three"""
    out = []
    for n in (0, 1, 3, 17):
        F = sphere_front(n, np.random.default_rng(900 + n))
        mid = F[n // 2] if n else np.array(REF3)
        for z in (3.0, 8.0, 15.0, 22.0, 30.0, 35.0):
            sd = np.array([0.02, 0.03, 0.025])
            # far below ref in f1 alone (the others above the front), below ref in all three, and under the middle of the front
            out.append((f"n{n}_one_z{z:g}", F, np.array([REF3[0] - z * sd[0], 0.9, 1.1]), np.array([sd[0], 0.05, 0.04])))
            out.append((f"n{n}_all_z{z:g}", F, np.array(REF3) - 0.55 * z * sd, sd))
            out.append((f"n{n}_under_z{z:g}", F, mid - 0.55 * z * sd, sd))
    return out


def narrow_case():
    """(name, front, mu, s): front points 1e-9 apart in f1 — boxes a billion times narrower than the belief"""
    F = R.pareto_front3([[0.5, 0.6, 0.7], [0.5 + 1e-9, 0.6 - 1e-3, 0.7 - 1e-3], [0.5 + 2e-9, 0.3, 0.65], [0.2, 0.9, 0.4], [0.9, 0.1, 0.2]], REF3)
    assert len(F) == 5
    return ("narrow_1e-9", F, np.array([0.5, 0.55, 0.6]), np.array([0.2, 0.15, 0.1]))
