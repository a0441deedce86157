"""Inputs of the knowledge-gradient envelope tests (tests/test_kg_host.py, tests/test_gpu_kg.py): families of lines (a, b) at which
an envelope construction can go wrong."""
import numpy as np


def random_lines(A, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(A), rng.standard_normal(A)


def concurrent(A, seed, z0=1.5, y0=0.25):
    """half the lines through the point (z0, y0): their breakpoints coincide up to rounding"""
    a, b = random_lines(A, seed)
    a[::2] = y0 - b[::2] * z0
    return a, b


def equal_slopes(A, seed):
    """half the lines share one slope"""
    a, b = random_lines(A, seed)
    b[::2] = b[0]
    return a, b


def grid(A, seed):
    """inputs on a coarse grid: exact ties in slope, in a, in both, and in the breakpoints"""
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, A) / 4.0, rng.integers(-6, 7, A) / 4.0


def far(z, extra=False):
    """a breakpoint at |z|; extra: a third line that adds an ordinary breakpoint behind it"""
    a, b = [0.0, -z * 1.25], [0.0, 1.25]
    if extra:
        a, b = a + [-z * 1.25 - 3.0], b + [2.5]
    return np.array(a), np.array(b)


def parabola(A):
    """tangents of a parabola, a = -b^2 / 2: every line is on the envelope"""
    b = np.linspace(-2.0, 2.0, A) if A > 1 else np.zeros(1)
    return -0.5 * b * b, b


def small_cases():
    """about 40 cases with A <= 64 for the 50-digit comparison: (name, a, b)"""
    out = []
    for A in (2, 3, 5, 8, 17, 33, 64):
        for seed in (1, 2):
            out.append((f"random_{A}_{seed}", *random_lines(A, 100 * A + seed)))
    for A in (4, 16, 64):
        for z0 in (0.0, 1.5):
            out.append((f"concurrent_{A}_{z0}", *concurrent(A, 7 * A, z0)))
        for seed in (1, 2):
            out.append((f"equal_slopes_{A}_{seed}", *equal_slopes(A, 11 * A + seed)))
    for A in (8, 32, 64):
        for seed in (1, 2):
            out.append((f"grid_{A}_{seed}", *grid(A, 13 * A + seed)))
    for z in (5.3, 10.7, 20.1, 30.9, 34.7):
        out.append((f"far_{z}", *far(z)))
    for z in (-12.3, 27.3, -34.9):
        out.append((f"far3_{z}", *far(z, True)))
    return out
