"""Inputs of the expected-hypervolume-improvement tests: fronts on a concave curve in [0, 1]^2, the reference point REF below it, and
beliefs that put the value anywhere from order one down to 1e-280."""
import json
from pathlib import Path

import numpy as np

REF = (-0.1, -0.2)
GOLDEN = Path(__file__).resolve().parent / "golden" / "ehvi2d_reference.json"


def concave_front(n, rng):
    """n points of the quarter circle f1^2 + f2^2 = 1 at random f1 in (0.02, 0.98): ascending in f1, descending in f2"""
    x = np.sort(rng.uniform(0.02, 0.98, size=n))
    assert n < 2 or np.all(np.diff(x) > 0)
    return np.stack([x, np.sqrt(1.0 - x * x)], axis=1).reshape(n, 2)


def random_beliefs(M, rng):
    """mu ~ N(0.5, 0.6^2), log s ~ N(-1.5, 1.2^2), each objective"""
    mu = 0.5 + 0.6 * rng.standard_normal((M, 2))
    s = np.exp(-1.5 + 1.2 * rng.standard_normal((M, 2)))
    return mu[:, 0], s[:, 0], mu[:, 1], s[:, 1]


def golden_cases():
    """tests/golden/ehvi2d_reference.json: name, n, front, ref, mu, s, `reference` (the reference implementation's ehvi2d in double
    precision) and `exact` (the 50-digit value rounded to double)"""
    return json.loads(GOLDEN.read_text())["cases"]


def tail_cases():
    """(name, front, mu1, s1, mu2, s2): candidates deep inside the dominated region — the value falls to 1e-280 as the distance of
    mu below the front grows to 35 standard deviations in one objective, or about 25 in both"""
    out = []
    for n in (1, 3, 17, 64):
        F = concave_front(n, np.random.default_rng(900 + n))
        for k, z in enumerate((3.0, 8.0, 15.0, 22.0, 30.0, 35.0)):
            s = 0.02
            # far to the left of the front in f1 alone (f2 above it), and below it in both
            out.append((f"n{n}_left_z{z:g}", F, REF[0] - z * s, s, 0.9, 0.05))
            out.append((f"n{n}_both_z{z:g}", F, REF[0] - 0.7 * z * s, s, REF[1] - 0.7 * z * 0.03, 0.03))
            # under the middle of the front: dominated by it, above ref
            mid = F[n // 2]
            out.append((f"n{n}_under_z{z:g}", F, mid[0] - 0.7 * z * s, s, mid[1] - 0.7 * z * 0.03, 0.03))
    return out
