"""The three-objective expected hypervolume improvement (include/gpe_ehvi3.h) — what can be held WITHOUT a device:

* the C-ABI: a header of its own, exported by libgpengine.so, bound by limbo_amd._capi; the box kernel in the code object;
* the accuracy of the REFERENCE every other comparison leans on: tests/ehvi3_ref.py's numpy box sums (value and six partials)
  against the same quantities in 50-digit arithmetic over grid cells — another construction: no sweep, no boxes — on random, tail
  and narrow-box cases down to 1e-280.  The error is MEASURED: its worst is E_REF_EHVI3 below, and the bars of the device tests
  (tests/test_gpu_ehvi3.py) are multiples of it;
* that the definition is the reference implementation's: tests/golden/ehvi3d_reference.json holds its ehvi3d_sliceupdate's and
  ehvi3d_8term's outputs beside the 50-digit values; they agree within that implementation's own error on the file, recorded below;
* Monte Carlo, and the properties the construction promises;
* gpe_ehvi3_front (host only) against a quadratic-time front in plain python; gpe_ehvi3_boxes for each axis against the height
  field by brute force, and as the prepared-front check;
* the host path of the C++ drop-in (acqui/ehvi3.hpp below Params::gpu::min_n_for_gpu): tests/cpp/test_ehvi3_dropin, compiled here
  with the flags of tests/cpp/Makefile, against the reference on the beliefs the driver itself reports."""
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from limbo_amd import _capi
from tests import ehvi3_cases as C
from tests import ehvi3_ref as R

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("gpe_ehvi3_front", "gpe_ehvi3_boxes", "gpe_ehvi3_values", "gpe_ehvi3_batch", "gpe_ehvi3_phase_ms")
# worst relative error of ref_ehvi3 (value and each of the six partials, wherever the 50-digit number is >= 1e-280) against 50-digit
# arithmetic over reference_cases(), measured 2026-10-21: 1.3941e-10, the value of n1_one_z35 — one front point, mu 35 standard deviations
# below the reference point in f1 (a result near 1e-271; the same figure with no front at all): psi's f(z) = phi + z Phi loses about z^2 ulps to cancellation there, the
# same spot and the same figure as the two-objective reference's.  On the random sphere and lattice cases the worst is 6e-13, on the
# narrow-box case 3e-16
E_REF_EHVI3 = 1.40e-10
BAR = 16 * E_REF_EHVI3  # the device's bar: the family's factor, for the device's own erfc / exp and another summation order: 2.2e-9
# The reference implementation's ehvi3d_sliceupdate and ehvi3d_8term against the 50-digit column of the golden file, measured on that
# file 2026-10-21.  Both subtract products of psi and Phi cell by cell, so their error is ABSOLUTE: relative to the value it is at
# most 1.7e-10 where the value is >= 1e-6 (3.3e-12 on multitest.txt, whose values are 9 to 47), and below 1e-6 it is at most 1.5e-16
# in plain units — they return 0 for the three cases at 5e-27, 5e-25 and 4e-22 (which the rule "value >= 1e-6 psi1(r1) psi2(r2)
# psi3(r3)" admits: there the product is tiny too).  The two schemes differ from each other by less than either does from 50 digits.
E_GOLDEN3_REL = 1.7e-10  # where the value is >= 1e-6
E_GOLDEN3_ABS = 1.5e-16  # where it is not


def rel_err(got, ref):
    """max relative difference where the reference is a normal number; elsewhere `got` must be as small"""
    got, ref = np.asarray(got, dtype=float).ravel(), np.asarray(ref, dtype=float).ravel()
    big = ref >= 1e-280
    assert np.all(got >= 0) and np.all(got[~big] <= 1e-279)
    return float(np.max(np.abs(got[big] - ref[big]) / ref[big])) if big.any() else 0.0


def golden(c):
    return np.array(c["front"], dtype=float).reshape(-1, 3), tuple(c["ref"]), np.array(c["mu"]), np.array(c["s"])


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_abi_lives_in_its_own_header(engine_lib):
    hs = (ROOT / "include" / "gpe_ehvi3.h").read_text()
    h = (ROOT / "include" / "gpe.h").read_text()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hs), n + " is not declared in include/gpe_ehvi3.h"
        assert not re.search(r"\b" + n + r"\s*\(", h), n + " must not be declared in include/gpe.h"
        assert hasattr(engine_lib.cdll, n), n + " is not exported by libgpengine.so"
        assert engine_lib.fn(n[4:]).argtypes is not None, n + " is not bound by _capi"
    assert '#include "gpe.h"' in hs
    for m in ("ehvi3_values", "ehvi3_batch", "ehvi3_phase_ms"):
        assert callable(getattr(_capi.Handle, m))
    assert callable(_capi.ehvi3_front) and callable(_capi.ehvi3_boxes)
    assert _capi.EHVI3_MAX_FRONT == 1024
    assert re.search(r"#define\s+GPE_EHVI3_MAX_FRONT\s+1024\b", hs)
    assert b"k_ehvi3" in _capi.ENGINE_SO.read_bytes(), "the box kernel is in the shipped code object"


# ------------------------------------------------------------------------------------------------ the reference's own accuracy
def reference_cases():
    """(name, front, mu, s): random beliefs on sphere and lattice fronts of n in {0, 1, 2, 3, 17, 24}, the tail cases, the narrow case"""
    out = []
    rng = np.random.default_rng(31)
    for n in (0, 1, 2, 3, 17, 24):
        F = C.sphere_front(n, rng)
        mu, s = C.random_beliefs(4, rng)
        out += [(f"sphere_n{n}_{k}", F, mu[k], s[k]) for k in range(4)]
    F = C.lattice_front(60, 8, rng)
    mu, s = C.near_beliefs(F, 4, rng)
    out += [(f"lattice_n{len(F)}_{k}", F, mu[k], s[k]) for k in range(4)]
    return out + C.tail_cases() + [C.narrow_case()]


def test_reference_against_50_digits():
    import mpmath as mp

    worst, smallest, setter = 0.0, 1.0, None
    for name, F, mu, s in reference_cases():
        v, p = R.ref_ehvi3(F, C.REF3, mu, s)
        ev, ep = R.mp_ehvi3(F, C.REF3, mu, s)
        errs = []
        for got, exact in zip([v[0]] + list(p[0]), [ev] + ep):
            assert got >= 0
            if exact >= mp.mpf("1e-280"):
                errs.append(float(abs(mp.mpf(float(got)) - exact) / exact))
            else:
                assert got <= 1e-279
        if ev >= mp.mpf("1e-280"):
            smallest = min(smallest, float(ev))
        print(f"{name:20s} ehvi = {mp.nstr(ev, 6):>14s}  worst relative error {max(errs) if errs else 0.0:.3e}")
        if errs and max(errs) > worst:
            worst, setter = max(errs), name
    print(f"worst relative error {worst:.4e} at {setter} (E_REF_EHVI3 = {E_REF_EHVI3:.4e}), smallest value held {smallest:.3e}")
    assert smallest <= 1e-270, "tail cases down to 1e-280 are among the cases"
    assert worst <= E_REF_EHVI3


def test_golden_file_pins_the_definition():
    """every case of the file, none skipped: the reference implementation's two schemes against the 50-digit sum over grid cells, and
    the file's 50-digit column against mp_ehvi3 as it is today"""
    cases = C.golden_cases()
    assert len(cases) == 40 and sorted({c["n"] for c in cases}) == [0, 1, 2, 3, 4, 17, 64, 65]
    assert {"multitest_0", "multitest_1", "multitest_2", "multitest_3", "simpletest"} <= {c["name"] for c in cases}
    worst_abs = worst_rel = 0.0
    for c in cases:
        F, ref, mu, s = golden(c)
        assert R.is_prepared3(F, ref) and len(F) == c["n"]
        exact, _ = R.mp_ehvi3(F, ref, mu, s, partials=False)
        base, _ = R.mp_ehvi3(np.zeros((0, 3)), ref, mu, s, partials=False)
        assert float(exact) == c["exact"] and exact >= 1e-6 * base, c["name"]
        v, _ = R.ref_ehvi3(F, ref, mu, s)
        assert abs(v[0] - c["exact"]) <= E_REF_EHVI3 * c["exact"], c["name"]
        for scheme in ("sliceupdate", "8term"):
            a = abs(c[scheme] - c["exact"])
            if c["exact"] >= 1e-6:
                worst_rel = max(worst_rel, a / c["exact"])
                assert a <= E_GOLDEN3_REL * c["exact"], (c["name"], scheme)
            else:
                worst_abs = max(worst_abs, a)
                assert a <= E_GOLDEN3_ABS, (c["name"], scheme)
    print(f"reference implementation against 50 digits: worst relative (value >= 1e-6) {worst_rel:.3e}, worst absolute below {worst_abs:.3e}")


MC_CASES = [(0, (0.3, 0.2, 0.1), (0.4, 0.5, 0.3)), (1, (0.6, 0.7, 0.5), (0.3, 0.2, 0.25)), (3, (0.2, 0.9, 0.5), (0.5, 0.3, 0.4)),
            (17, (0.7, 0.6, 0.65), (0.25, 0.35, 0.3))]


@pytest.mark.parametrize("n,mu,s", MC_CASES)
def test_reference_against_monte_carlo(n, mu, s):
    F = C.sphere_front(n, np.random.default_rng(50 + n))
    v, _ = R.ref_ehvi3(F, C.REF3, mu, s)
    mean, se = R.mc_hvi3(F, C.REF3, mu, s, draws=1_000_000, seed=n)
    print(f"n = {n}: ehvi {v[0]:.6e}, Monte Carlo {mean:.6e} +- {se:.1e} ({(v[0] - mean) / se:+.2f} standard errors)")
    assert se > 0 and abs(v[0] - mean) <= 4 * se


def test_reference_properties():
    rng = np.random.default_rng(7)
    for F in (C.sphere_front(17, rng), C.lattice_front(50, 7, rng)):
        mu, s = C.near_beliefs(F, 200, rng)
        v, p = R.ref_ehvi3(F, C.REF3, mu, s)
        assert np.all(v >= 0) and np.all(p >= 0), "EHVI and its partials (sums of positive terms) are >= 0"
        # the three tables give one value
        for c in (0, 1):
            assert rel_err(R.ref_ehvi3(F, C.REF3, mu, s, value_axis=c)[0], v) <= E_REF_EHVI3
        # n = 0: the product of the three one-sided expected improvements; one more front point never raises a value
        v0, _ = R.ref_ehvi3(np.zeros((0, 3)), C.REF3, mu, s)
        psi = [R._ev(mu[:, k], s[:, k], np.array([C.REF3[k]]))[0][:, 0] for k in range(3)]
        assert np.max(np.abs(v0 - psi[0] * psi[1] * psi[2]) / v0) <= 1e-14
        assert np.all(v <= v0 * (1 + 1e-12) + 1e-300)
        for k in (0, len(F) // 2, len(F) - 1):
            less, _ = R.ref_ehvi3(np.delete(F, k, axis=0), C.REF3, mu, s)
            assert np.all(v <= less * (1 + 1e-12) + 1e-300)
        # the boxes of each table: at most 2n + 1, exactly as many in general position
        counts = [len(R.boxes3(F, C.REF3, c)) for c in range(3)]
        assert all(k <= 2 * len(F) + 1 for k in counts) and (len(np.unique(F)) < F.size or counts == [2 * len(F) + 1] * 3)
        # s = 0 in all three: the plain hypervolume improvement of the point mu
        vz, _ = R.ref_ehvi3(F, C.REF3, mu, np.zeros_like(s))
        hv = R.hypervolume3(F, C.REF3)
        for m in range(0, len(mu), 4):
            G = R.pareto_front3(np.vstack([F, mu[m:m + 1]]), C.REF3)
            assert abs(vz[m] - (R.hypervolume3(G, C.REF3) - hv)) <= 1e-14, m
        assert np.max(np.abs(vz - R.hvi_points3(F, C.REF3, mu))) <= 1e-15
        assert np.any(vz > 0) and np.any(vz == 0)


def test_dominated_point_changes_nothing(engine_lib):
    """a dominated point, a duplicate and a point below ref added before gpe_ehvi3_front: the same front, hence the same tables"""
    rng = np.random.default_rng(12)
    F = C.sphere_front(17, rng)
    extra = np.vstack([F[5] - [0.01, 0.0, 0.02], F[9], [0.5, C.REF3[1], 0.5], 0.3 * F[2]])
    rc, G = _capi.ehvi3_front(np.vstack([extra[:2], F[::-1], extra[2:]]), C.REF3)
    assert rc == 0 and np.array_equal(G, F)
    for c in range(3):
        assert np.array_equal(_capi.ehvi3_boxes(G, C.REF3, c)[1], R.boxes3(F, C.REF3, c))


def test_partials_against_central_differences_of_50_digits():
    """the six partials of the reference against central differences of the VALUE as the 50-digit checker forms it — step 1e-20, and
    100 digits for the difference itself: a partial can be 1e-40 of the value, which 50 digits minus the step's 20 would not
    resolve.  The truncation error is 1e-40 f''', far below the bar."""
    import mpmath as mp

    rng = np.random.default_rng(11)
    worst, held = 0.0, 0
    for n in (0, 1, 3, 17):
        F = C.sphere_front(n, rng)
        mu, s = C.near_beliefs(F, 4, rng)
        _, p = R.ref_ehvi3(F, C.REF3, mu, s)
        for m in range(4):
            _, mp_p = R.mp_ehvi3(F, C.REF3, mu[m], s[m])
            with mp.workdps(100):
                h = mp.mpf("1e-20")

                def val(k, t):
                    x = [mp.mpf(float(q)) for q in list(mu[m]) + list(s[m])]
                    x[k] += t
                    return R.mp_ehvi3(F, C.REF3, x[:3], x[3:], partials=False, dps=100)[0]

                for c in range(3):
                    for which, k in ((0, c), (1, 3 + c)):
                        cd = (val(k, h) - val(k, -h)) / (2 * h)
                        if cd < mp.mpf("1e-280"):
                            continue
                        held += 1
                        assert abs(mp_p[2 * c + which] - cd) / cd <= mp.mpf("1e-18"), "mp_ehvi3's partials are the value's derivatives"
                        worst = max(worst, float(abs(mp.mpf(float(p[m, 2 * c + which])) - cd) / cd))
    print(f"partials against central differences of the 50-digit value: {held} held, worst relative error {worst:.3e}")
    assert held >= 90 and worst <= E_REF_EHVI3


# ------------------------------------------------------------------------------------------------ gpe_ehvi3_front, gpe_ehvi3_boxes
def test_front_preparation(engine_lib):
    rng = np.random.default_rng(3)
    ref = (0.1, 0.2, 0.15)
    for n in (0, 1, 2, 9, 100, 3000):
        P = rng.uniform(0, 1, size=(n, 3))  # dominated points, points at or below ref, unsorted
        if n >= 100:
            P[10:60] = np.round(P[10:60] * 5) / 5  # ties in each coordinate, duplicates
        if n >= 9:
            P[3] = P[1]  # a duplicate
            P[4] = (ref[0], 0.9, 0.9)  # on ref in f1
            P[5] = (0.95, ref[1], 0.9)  # on ref in f2
            P[6] = (0.95, 0.9, ref[2] - 0.1)  # below ref in f3
            P[7] = (np.inf, 0.5, 0.5)  # not finite: dropped
            P[8] = (-np.inf, 0.5, 0.5)
            P[2] = (P[0, 0], P[0, 1], P[0, 2] - 0.01)  # equal in f1 and f2, lower in f3: dominated
        rc, F = _capi.ehvi3_front(P, ref)
        assert rc == 0
        assert len(F) > _capi.EHVI3_MAX_FRONT or _capi.ehvi3_boxes(F, ref, 2, check=False)[0] == 0, "what it returns is prepared"
        if n <= 100:
            assert np.array_equal(F, R.pareto_front3(P, ref)), n
        else:  # every kept point is one of P's, the order is right, none dominates another, every point of P above ref is dominated or kept
            keep = {tuple(p) for p in F}
            assert keep <= {tuple(p) for p in P} and len(keep) == len(F)
            assert [tuple(p) for p in F] == sorted(keep, key=lambda p: (-p[2], p[0], p[1]))
            for p in P:
                if np.all(np.isfinite(p)) and np.all(p > ref):
                    dom = np.all(F >= p[None, :], axis=1)
                    assert dom.sum() >= 1 and (tuple(p) not in keep or dom.sum() == 1)
    # duplicates of one point: one is kept
    rc, F = _capi.ehvi3_front(np.tile([[0.5, 0.6, 0.7]], (9, 1)), ref)
    assert rc == 0 and F.tolist() == [[0.5, 0.6, 0.7]]
    # a NaN is GPE_ERR_ARG, in the points and in ref
    P = rng.uniform(0.3, 1, size=(5, 3))
    P[2, 1] = np.nan
    assert _capi.ehvi3_front(P, ref, check=False)[0] == -1
    assert _capi.ehvi3_front(P[:2], (np.nan, 0.0, 0.0), check=False)[0] == -1
    assert _capi.ehvi3_front(P[:2], (np.inf, 0.0, 0.0), check=False)[0] == -1


def check_table(F, ref, c, B):
    """B against the height field by brute force on the grid of the front's coordinates: every cell of the grid lies in exactly one
    row (disjoint, covering [r_a, inf) x [r_b, inf)), whose height is the cell's; the rows' ends are grid lines.  A row's lower corner
    is the lower corner of a cell — the rows are half-open — so its height is h_c of that cell: the points with f_a > l_a, f_b > l_b."""
    xa, xb, H = R.height_grid(F, ref, c)
    assert len(B) <= 2 * len(F) + 1 and len(B) >= 1
    ends_a, ends_b = set(xa.tolist()) | {np.inf}, set(xb.tolist()) | {np.inf}
    owner = np.full(H.shape, -1)
    for k, (la, ua, lb, ub, h) in enumerate(B):
        assert la < ua and lb < ub and {la, ua} <= ends_a and {lb, ub} <= ends_b
        ia, ib = (xa >= la) & (xa < ua), (xb >= lb) & (xb < ub)
        assert np.all(owner[np.ix_(ia, ib)] == -1), "two rows overlap"
        owner[np.ix_(ia, ib)] = k
        assert np.all(H[np.ix_(ia, ib)] == h), "a row's height is the height field's over all of it"
        assert H[np.searchsorted(xa, la), np.searchsorted(xb, lb)] == h
    assert np.all(owner >= 0), "the rows cover the quadrant"


def test_boxes_against_the_height_field(engine_lib):
    rng = np.random.default_rng(21)
    fronts = [np.zeros((0, 3)), C.sphere_front(1, rng), C.sphere_front(2, rng), C.sphere_front(33, rng), C.sphere_front(195, rng),
              C.lattice_front(60, 8, rng), C.lattice_front(300, 12, rng), C.lattice_front_with_boxes(64), C.narrow_case()[1]]
    for F in fronts:
        general = len(np.unique(F)) == F.size
        for c in range(3):
            rc, B = _capi.ehvi3_boxes(F, C.REF3, c)
            assert rc == 0
            check_table(F, C.REF3, c, B)
            assert np.array_equal(B, R.boxes3(F, C.REF3, c)), "the rows' order is the sweep's: a function of the front alone"
            assert not general or len(B) == 2 * len(F) + 1
            # a cap the table does not fit: refused, nothing written
            assert _capi.ehvi3_boxes(F, C.REF3, c, cap=len(B) - 1, check=False)[0] == -1
    assert len(_capi.ehvi3_boxes(C.lattice_front_with_boxes(64), C.REF3, 2)[1]) == 64


def test_boxes_refuse_a_front_that_is_not_prepared(engine_lib):
    rng = np.random.default_rng(22)
    G = C.sphere_front(9, rng)
    bad = lambda F, ref=C.REF3, axis=2: _capi.ehvi3_boxes(F, ref, axis, check=False)[0] == -1
    values_check = lambda F, ref=C.REF3: engine_lib.fn("ehvi3_values")(
        None, _capi._d(np.ascontiguousarray(F)), len(F), _capi._d(np.asarray(ref, dtype=float)), None, None, 0, None, None)
    assert not bad(G) and values_check(G) == 0 and values_check(np.zeros((0, 3))) == 0
    T = np.array([[0.5, 0.6, 0.7], [0.6, 0.5, 0.7], [0.4, 0.4, 0.7 - 1e-3]])  # ties in f3: ascending in f1; the third is dominated
    assert not bad(T[:2]) and bad(T[[1, 0]]), "ties in f3 ascend in f1"
    for axis in range(3):
        assert bad(G[::-1], axis=axis), "ascending in f3"
        assert bad(G[[0, 2, 1, 3]], axis=axis), "unsorted"
        assert bad(np.vstack([G[:3], G[2:3], G[3:]]), axis=axis), "a duplicate"
        assert bad(T, axis=axis), "a dominated point behind its dominator"
        assert not bad(np.vstack([[[0.45, 0.55, 0.75]], T[:2]]), axis=axis)
        assert not bad(np.array([[0.3, 0.3, 0.75], [0.5, 0.6, 0.7]]), axis=axis)
        assert bad(np.array([[0.3, 0.3, 0.75], [0.5, 0.6, 0.75]]), axis=axis), "a dominated point in front of its dominator (a tie in f3)"
        assert bad(G, ref=(G[:, 0].min(), C.REF3[1], C.REF3[2]), axis=axis), "a front point not above ref in f1"
        assert bad(G, ref=(C.REF3[0], C.REF3[1], G[-1, 2]), axis=axis), "a front point not above ref in f3"
        assert bad(G, ref=(np.nan, 0.0, 0.0), axis=axis) and bad(G, ref=(-np.inf, 0.0, 0.0), axis=axis)
        Gn = G.copy()
        Gn[4, 1] = np.nan
        assert bad(Gn, axis=axis)
        Gn[4, 1] = np.inf
        assert bad(Gn, axis=axis)
    assert bad(G, axis=3) and bad(G, axis=-1)
    assert values_check(G[::-1]) == -1 and values_check(T) == -1
    big = C.sphere_front(_capi.EHVI3_MAX_FRONT + 1, rng)
    assert bad(big) and values_check(big) == -1, "n > GPE_EHVI3_MAX_FRONT"
    assert not bad(big[1:]) and values_check(big[1:]) == 0


# ------------------------------------------------------------------------------------------------ the drop-in's host path
DRIVER = ROOT / "tests" / "cpp" / "test_ehvi3_dropin"
NOISES = (0.01, 0.1)  # Params::kernel::noise of the driver by noise_id
FD_STEP = 1e-4


def build_driver():
    """tests/cpp/test_ehvi3_dropin with the flags of tests/cpp/Makefile (that file is not this test's to change)"""
    src = DRIVER.with_suffix(".cpp")
    deps = [src, _capi.ENGINE_SO] + list((ROOT / "include").rglob("*.h*"))
    if DRIVER.exists() and all(DRIVER.stat().st_mtime >= d.stat().st_mtime for d in deps):
        return DRIVER
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Wno-unused-variable", "-I" + str(ROOT / "include" / "limbo_amd"),
                           "-I" + str(ROOT / "oracle" / "ref_build" / "shim"), "-o", str(DRIVER), str(src), "-L" + str(ROOT / "limbo_amd"),
                           "-lgpengine", "-Wl,-rpath,$ORIGIN/../../limbo_amd", "-Wl,-rpath,/opt/rocm/lib", "-lpthread"])
    return DRIVER


def run_driver(tmp_path, kind, mean, X, Y, Fp, ref, Q, noise_id=0, observation=0, hp=None, env=None):
    exe = build_driver()
    n, D = X.shape
    f = tmp_path / "in.txt"
    with open(f, "w") as fh:
        fh.write(f"{kind} {mean} {D} {n} {len(Fp)} {len(Q)} {noise_id} {int(observation)} {0 if hp is None else len(hp)} "
                 f"{ref[0]!r} {ref[1]!r} {ref[2]!r}\n")
        if hp is not None:
            fh.write(" ".join(repr(float(v)) for v in hp) + "\n")
        for i in range(n):
            fh.write(" ".join(repr(float(v)) for v in list(X[i]) + list(Y[i])) + "\n")
        for v in list(Fp) + list(Q):
            fh.write(" ".join(repr(float(x)) for x in v) + "\n")
    r = subprocess.run([str(exe), str(f)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        out[w[0]] = np.array([float(v) for v in w[1:]])
    return out


def dropin_problem(kind, n, M, seed):
    """three competing objectives of x in [0, 1]^D with noise; the front is taken from the observations themselves"""
    D = 3 if kind == 0 else 2
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, size=(n, D))
    t = 1.5 * X.sum(axis=1)
    Y = np.stack([np.cos(t) + 0.3 * X[:, 0], np.sin(t) - 0.3 * X[:, 0], np.cos(t + 2.0) + 0.4 * X[:, 1]], axis=1) + 0.05 * rng.normal(size=(n, 3))
    ref = tuple(float(Y[:, k].min()) - 0.1 for k in range(3)) if n else (0.5, 0.2, 0.3)
    return X, Y, ref, rng.uniform(-0.3, 1.3, size=(M, D))  # (beyond the data: beliefs wide enough for values that do not vanish)


def with_steps(Q, h=FD_STEP):
    """Q followed by Q + h e_d and Q - h e_d for every d: one driver run gives batch() on all of them"""
    M, D = Q.shape
    out = [Q]
    for d in range(D):
        e = np.zeros(D)
        e[d] = h
        out += [Q + e, Q - e]
    return np.vstack(out)


def sd_of(s2, noise, observation):
    return np.sqrt(s2 if observation else np.maximum(s2 - noise, 0.0))


def check_dropin(got, M, D, noise, observation, bar, what):
    """the driver's numbers against the reference ON THE BELIEFS THE DRIVER REPORTS, and its gradients against central differences
    of its own batch().  bar: relative, on the values.  The gradient: step h = 1e-4 — truncation h^2 f''' / 6 = 2e-9 f''' plus rounding
    1e-16 / h — against 1e-6 max(1, |grad|): three orders of room for f''' and still six digits of the gradient."""
    T = M * (1 + 2 * D)
    front = got["front"].reshape(-1, 3)
    ref = got["ref_used"]
    assert R.is_prepared3(front, ref) and abs(got["hv"][0] - R.hypervolume3(front, ref)) <= 1e-13 * max(1.0, got["hv"][0])
    mu, s2 = got["mu"].reshape(T, 3, order="F"), got["s2"]
    sd = sd_of(s2, noise, observation)
    one, _ = R.ref_ehvi3(front, ref, mu, np.stack([sd] * 3, axis=1))
    e1 = rel_err(got["one"], one)
    mu3 = np.stack([got["mu1"], got["mu2"], got["mu3"]], axis=1)
    sd3 = np.stack([sd_of(got[f"s2_{k}"], noise, observation) for k in (1, 2, 3)], axis=1)
    three, part = R.ref_ehvi3(front, ref, mu3, sd3)
    e3 = rel_err(got["three"], three)
    print(f"{what}: ehvi in [{one.min():.3e}, {one.max():.3e}], median {np.median(one):.3e}; relative error: one model {e1:.3e}, three {e3:.3e}")
    assert e1 <= bar and e3 <= bar
    assert int(got["best_one"][0]) == int(np.argmax(got["one"])) and int(got["best_three"][0]) == int(np.argmax(got["three"]))
    assert int(got["best_none"][0]) == -1
    assert np.array_equal(got["obj"], got["three"]), "the objective's batch() is batch()"
    assert rel_err(got["val"], got["three"]) <= bar, "batch_grad's values are batch()'s (beliefs from query_grad_batch, not query_batch)"
    g = got["grad"].reshape(T, D)[:M]
    val = got["val"]
    cd = np.stack([(val[M * (1 + 2 * d):M * (2 + 2 * d)] - val[M * (2 + 2 * d):M * (3 + 2 * d)]) / (2 * FD_STEP) for d in range(D)], axis=1)
    dg = float(np.max(np.abs(g - cd)))
    print(f"{what}: max|grad| {np.max(np.abs(g)):.3e}, max|grad - central difference| {dg:.3e}")
    assert np.max(np.abs(g)) > 1e-4, "a gradient that is zero everywhere shows nothing"
    assert dg <= 1e-6 * max(1.0, float(np.max(np.abs(g))))
    assert abs(got["single"][0] - val[0]) <= bar * val[0] and np.max(np.abs(got["single"][1:] - g[0])) <= 1e-6 * max(1.0, float(np.max(np.abs(g))))
    if "search_value" in got:  # opt::BatchGradSearch climbs it: no worse than the best of its own starts
        assert got["search_value"][0] >= np.max(got["search_starts"]) * (1 - 1e-12) and got["search_value"][0] > 0
        print(f"{what}: BatchGradSearch: best start {np.max(got['search_starts']):.6e}, returned {got['search_value'][0]:.6e}")
    return one, three, part


# (kind, mean, n, noise_id, observation): SE-ARD with the Data mean, latent; Matern-5/2, the observation's variance; a constant mean
HOST_CASES = [(0, 0, 60, 0, 0), (1, 0, 40, 1, 1), (0, 2, 200, 0, 0)]
HOST_ENV = {"LIMBO_AMD_MIN_N_FOR_GPU": str(1 << 20), "LIMBO_AMD_HOST_BATCH_CROSSOVER": str(1 << 40)}


@pytest.mark.parametrize("kind,mean,n,noise_id,observation", HOST_CASES)
def test_dropin_host_path(tmp_path, kind, mean, n, noise_id, observation):
    M = 12
    X, Y, ref, Q = dropin_problem(kind, n, M, 100 * kind + 10 * mean + n)
    got = run_driver(tmp_path, kind, mean, X, Y, Y, ref, with_steps(Q), noise_id, observation, env=HOST_ENV)
    assert np.all(got["host_resident"] == 1)
    got["ref_used"] = ref
    assert np.array_equal(got["front"].reshape(-1, 3), R.pareto_front3(Y, ref))
    one, _, _ = check_dropin(got, M, Q.shape[1], NOISES[noise_id], observation, 10 * E_REF_EHVI3, f"host n = {n}")
    assert np.mean(one >= 1e-6) >= 0.25, "values that all vanish show little"
    assert "search_value" in got


def test_dropin_prior(tmp_path):
    """no samples: the prior's beliefs (mean functor, k(v, v)), an empty front: the product of three expected improvements"""
    Q = np.random.default_rng(5).uniform(0, 1, size=(6, 3))
    ref = (0.5, 0.2, 0.3)
    got = run_driver(tmp_path, 0, 2, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), ref, with_steps(Q), env=HOST_ENV)
    assert got["front"].size == 0 and got["hv"][0] == 0.0
    mu, s2 = got["mu"].reshape(-1, 3, order="F"), got["s2"]
    sd = np.stack([sd_of(s2, NOISES[0], 0)] * 3, axis=1)
    want, _ = R.ref_ehvi3(np.zeros((0, 3)), ref, mu, sd)
    assert rel_err(got["one"], want) <= 10 * E_REF_EHVI3 and rel_err(got["three"], want) <= 10 * E_REF_EHVI3
    assert np.all(got["one"] > 0)
