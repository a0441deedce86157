"""The sparse pseudo-input GP (include/gpe_sparse.h) without a GPU: the ABI (a header of its own, exported by libgpengine.so, bound
by limbo_amd._capi, gpe.h's symbol set untouched), the launch plan of the weighted Gram executed in numpy, the argument checks
that touch no device, and the two numpy references of tests/sparse_ref.py against each other."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from limbo_amd import _capi
from tests import sparse_ref as R

ROOT = Path(__file__).resolve().parent.parent
TILE, KSTEP = 64, 4  # the Gram's tile edge; the k step of v_mfma_f64_16x16x4_f64
ENTRIES = """gpe_sp_create gpe_sp_destroy gpe_sp_last_error gpe_sp_set_data gpe_sp_set_pseudo gpe_sp_set_hparams gpe_sp_compute
gpe_sp_nlml gpe_sp_objective gpe_sp_predict gpe_sp_get_L gpe_sp_get_Lm gpe_sp_get_bet gpe_sp_get_ep gpe_sp_set_profiling
gpe_sp_phase_ms gpe_debug_gram_plan""".split()


def _declared(header):
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / header).read_text(), flags=re.S)
    return set(re.findall(r"\b(gpe_[A-Za-z0-9_]+)\s*\(", txt))


def test_header_exports_and_binding():
    dec = _declared("gpe_sparse.h")
    assert dec == set(ENTRIES)
    assert not (dec & _declared("gpe.h"))  # tests/test_abi.py holds the oracle to gpe.h: the new entries stay out of it
    raw = ctypes.CDLL(str(_capi.ENGINE_SO))  # the dynamic symbol table itself, not the binding's view of it
    for name in ENTRIES:
        assert hasattr(raw, name), name
    lib = _capi.load_engine()
    for name in ENTRIES:
        assert lib.fn(name[len("gpe_"):]).argtypes is not None, name
    for m in ("set_data", "set_pseudo", "set_hparams", "compute", "nlml", "objective", "predict", "get_L", "get_Lm", "get_bet", "get_ep",
              "phase_ms"):
        assert hasattr(_capi.SparseHandle, m), m


@pytest.mark.parametrize("chunk", [0, 512], ids=["chunk_default", "chunk512"])
@pytest.mark.parametrize("N", [1300, 5000, 200000])
@pytest.mark.parametrize("M", [40, 193, 320, 1024, 4096])
def test_gram_plan_covers_every_tile_and_k_once(M, N, chunk):
    lib = _capi.load_engine()
    plan = _capi.debug_gram_plan(lib, M, N, chunk, 256)
    nt = (M + TILE - 1) // TILE
    ti, tj, k0, k1, slot = plan.T
    assert np.all((0 <= tj) & (tj <= ti) & (ti < nt))
    assert np.all(k0 % KSTEP == 0) and np.all((0 <= k0) & (k0 < k1) & (k1 <= N))
    tile = ti * (ti + 1) // 2 + tj
    order = np.lexsort((slot, tile))  # by tile, then by slot: the order a tile's partial products are added in
    t_s, k0_s, k1_s, slot_s = tile[order], k0[order], k1[order], slot[order]
    first = np.r_[True, t_s[1:] != t_s[:-1]]
    last = np.r_[first[1:], True]
    assert np.array_equal(np.unique(tile), np.arange(nt * (nt + 1) // 2))  # every lower tile is there
    assert np.all(k0_s[first] == 0) and np.all(k1_s[last] == N)            # ... from column 0 to column N
    inner = ~first
    assert np.all(k0_s[inner] == k1_s[:-1][inner[1:]])                     # ... without a gap or an overlap
    assert np.all(slot_s[inner] > slot_s[:-1][inner[1:]])                  # a tile's slots ascend with k0
    # launch order: a chunk's workgroups are contiguous, and no chunk of the stream is longer than asked
    if chunk:
        assert np.all(k1 - k0 <= chunk) and np.all(k0 // chunk == (k1 - 1) // chunk)


@pytest.mark.parametrize("M,N,chunk", [(40, 1300, 0), (193, 1300, 512), (320, 5000, 512), (320, 5000, 0), (1024, 5000, 512), (1024, 5000, 0)])
def test_gram_plan_executed_in_numpy(M, N, chunk):
    """the plan's rows, run as tile products in the order of the fold (ascending slot), reproduce Z^T diag(w) Z"""
    lib = _capi.load_engine()
    plan = _capi.debug_gram_plan(lib, M, N, chunk, 256)
    rng = np.random.default_rng(M + N)
    Z = rng.standard_normal((N, M))
    w = rng.random(N) + 0.5
    A = np.zeros((M, M))
    for ti, tj, k0, k1, _ in plan[np.argsort(plan[:, 4], kind="stable")]:
        r, c = slice(ti * TILE, min((ti + 1) * TILE, M)), slice(tj * TILE, min((tj + 1) * TILE, M))
        A[r, c] += (Z[k0:k1, r] * w[k0:k1, None]).T @ Z[k0:k1, c]
    ref = (Z * w[:, None]).T @ Z
    low = np.tril(np.ones((M, M), dtype=bool))
    blk = np.kron(np.tril(np.ones(((M + TILE - 1) // TILE,) * 2, dtype=bool)), np.ones((TILE, TILE), dtype=bool))[:M, :M]
    assert np.all(A[~blk] == 0.0)  # nothing above the lower tiles
    err = np.max(np.abs(A - ref)[low]) / np.max(np.abs(ref))
    print(f"M={M} N={N} chunk={chunk}: {len(plan)} workgroups, max rel err {err:.2e}")
    assert err <= 1e-13


def test_bad_arguments_return_minus_one():
    lib = _capi.load_engine()
    f = lib.fn("debug_gram_plan")
    assert f(0, 1000, 0, 256, None, 0) == -1
    assert f(64, 0, 0, 256, None, 0) == -1
    assert f(64, 1000, 0, 0, None, 0) == -1
    assert f(-5, -5, 512, 256, None, 0) == -1
    assert f(64, 1000, 0, 256, None, 0) > 0
    # entry points refuse null handles and null outputs before they touch a device
    assert lib.fn("sp_create")(0, None) == -1
    for name, args in (("sp_compute", ()), ("sp_destroy", ()), ("sp_set_pseudo", (None, 4)), ("sp_set_data", (None, 4, 2, None, 1)),
                       ("sp_set_hparams", (None, 0.0, 0.0, 1e-6)), ("sp_nlml", (None,)), ("sp_predict", (None, 4, None, None)),
                       ("sp_get_L", (None, 4)), ("sp_get_Lm", (None, 4)), ("sp_get_bet", (None,)), ("sp_get_ep", (None,)),
                       ("sp_phase_ms", (None,)), ("sp_objective", (None, 0.0, 0.0, 1e-6, None))):
        assert lib.fn(name)(None, *args) == -1, name


@pytest.mark.parametrize("jitter", [1e-6, 1e-4])
@pytest.mark.parametrize("shape", [(1300, 128, 3, 1), (1400, 200, 6, 1)], ids=["n1300_m128_d3", "n1400_m200_d6"])
def test_reference_routes_agree_to_a_thousandth_of_the_bars(shape, jitter):
    """route (a), the reference's sequence, against route (b), the dense definition: the GPU tests' bars are 1e-8 absolute on mu
    and s2 and 1e-10 relative on the likelihood; the checker itself is held to a thousandth of each.  A thousandth of 1e-10 is
    1e-13 relative on |nlml| ~ 10^3 — a few hundred ulps of work in double: both routes therefore add their scalar sums in
    extended precision and (b) refines Sigma^-1 y once, and the two shapes (N 1300-1400, M 128-200, D 3 and 6, cond K_mm 1e5 ..
    1e6) are ones where the disagreement stays under 3e-14 whatever the BLAS thread count (measured with 1, 2, 4 and 8 threads
    when this was written: nlml 5e-15 .. 2.7e-14, mu 2.4e-13 .. 1.4e-12, s2 <= 3.4e-14)."""
    pr = R.make_problem(*shape, seed=7)
    d_mu, d_s2, d_lik, _ = R.disagreement(pr, jitter)
    print(f"{shape} jitter={jitter:g}: (a) against (b): |mu| {d_mu:.2e}  |s2| {d_s2:.2e}  nlml rel {d_lik:.2e}")
    assert d_mu <= 1e-11 and d_s2 <= 1e-11 and d_lik <= 1e-13
