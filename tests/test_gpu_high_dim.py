"""GPU tests above 16 input dimensions (run with -m gpu on an MI355X), and of the K that compute() actually factorises.

The kernels are compiled once per dimension bucket: k_build (get_K, query and add_sample cross kernels) DMAX 2 4 8 16 32 64,
k_build_wide (the K compute() factorises) 2 4 6 8 16 32 64, k_grad_tiles<DMAX, LAM, PM> 2 4 6 8 16 32 64 x PM 1 / 8 and LAM 4 8
16 32, k_row_density (sparsify) 8 16 32 64; the host picks the bucket from kp.D = input dimensions + Lambda columns.  The
problems come from tests/high_dim.py (length scales ~ sqrt(D), every dimension its own weight, the last one the heaviest);
tests/test_high_dim_problems.py shows on the CPU that a dropped or truncated dimension would fail these checks.

get_K runs k_build<DM, 1> (libm exp); compute() builds K with k_build_wide or generates its tiles inside k_tail (both on
kfun_fast.h's exp_nonpos) and never hands it back: L L^T against the reference K, entry by entry at 1e-13 max diag K, checks
that K about 100x more sharply than |L - L_ref| does.  Tolerances otherwise SURVEY.md §8(c), as tests/test_gpu_parity.py."""
import numpy as np
import pytest

from limbo_amd import _capi
from oracle import np_oracle as O
from tests import high_dim as HD
from tests import parity_checks as PC
from tests.util import new_gp, relerr, relerr_norm

pytestmark = pytest.mark.gpu


def _llt_err(L, K):
    return float(np.max(np.abs(L @ L.T - K)) / np.max(np.diag(K)))


# ------------------------------------------------------------------------------------------------------ 1. the K sweep
@pytest.mark.parametrize("kind", HD.KINDS, ids=lambda k: HD.KIND_NAMES[k])
def test_gpu_kernel_matrix_sweep(engine_lib, kind):
    """Every bucket of k_build<DM, 1> (get_K) and of the factorised K — k_build_wide (N = 100), tiles generated inside k_tail
    (N = 320), both (N = 333: ragged last block) — at D = 1 .. 62, both sides of every bucket edge: get_K against
    np_oracle.kernel_matrix at 5e-14 relative and exactly symmetric; L L^T against the same K at 1e-13 max diag K, entry by
    entry; a zero upper triangle.  One handle, reused through set_data / set_kernel."""
    h = _capi.Handle(engine_lib)
    bad = []
    for kd, N, D in HD.sweep_cases():
        if kd != kind:
            continue
        pb = HD.problem(kind, N, D)
        h.set_data(pb.X, pb.obs_mean)
        h.set_kernel(kind, pb.theta, pb.noise)
        K = O.kernel_matrix(kind, pb.X, pb.theta, pb.noise)
        Kg = h.get_K()
        ek = relerr(Kg, K, floor=1e-30)
        sym = np.array_equal(Kg, Kg.T)
        assert h.compute() == 0, (N, D)
        L = h.get_L()
        el = _llt_err(L, K)
        up = np.all(np.triu(L, 1) == 0.0)
        if not (ek < HD.K_BAR and sym and el < HD.LLT_BAR and up):
            bad.append(dict(N=N, D=D, get_K=ek, symmetric=sym, LLt=el, upper_zero=bool(up)))
    assert h.flow_retries() == 0
    h.close()
    assert not bad, bad


@pytest.mark.parametrize("kind,N,D", HD.big_cases(), ids=lambda v: str(v))
def test_gpu_kernel_matrix_big(engine_lib, kind, N, D):
    """N = 3392: k_build_wide builds K (t0 = 768), the tall and closing data-flow launches factorise it; 256 sampled columns of
    get_K and of L L^T against the reference K (test_gpu_parity.py::test_gpu_c2_full_size_properties' form, 1e-13 here)."""
    pb = HD.problem(kind, N, D)
    cols = HD.big_columns(N)
    Kc = HD.kernel_columns(kind, pb.X, pb.theta, pb.noise, cols)
    h = new_gp(engine_lib, kind, pb.X, pb.obs_mean, pb.theta, pb.noise)
    Kg = h.get_K()
    assert relerr(Kg[:, cols], Kc, floor=1e-30) < HD.K_BAR
    assert np.array_equal(Kg[:, cols], Kg[cols, :].T)
    del Kg
    assert h.compute() == 0
    L = h.get_L()
    assert np.all(np.triu(L, 1) == 0.0)
    assert np.max(np.abs(L @ L[cols].T - Kc)) < HD.LLT_BAR * np.max(Kc[cols, np.arange(cols.size)])
    assert h.flow_retries() == 0
    h.close()


# ------------------------------------------------------------------------------------------- 2. bitwise bucket invariance
def _everything(lib, pb, Xq):
    h = new_gp(lib, pb.kind, pb.X, pb.obs_mean, pb.theta, pb.noise)
    assert h.compute() == 0
    out = dict(L=h.get_L(), alpha=h.get_alpha(), ll=h.log_lik())
    out["kta"], out["var"] = h.query_batch(Xq)
    out["grad"] = h.log_lik_grad(True)
    assert h.flow_retries() == 0
    h.close()
    return out


@pytest.mark.parametrize("D", [p[0] for p in HD.INVARIANCE_PAIRS])
@pytest.mark.parametrize("kind", (O.SE_ARD, O.MATERN52), ids=lambda k: HD.KIND_NAMES[k])
def test_gpu_bucket_invariance_bitwise(engine_lib, kind, D):
    """A constant column appended to X and to the query points takes the problem from D to D + 1 dimensions — across a bucket
    edge of k_build / k_build_wide / k_grad_tiles, or to the top of the range (61 -> 62).  Its pair differences are exact
    zeros and the kernels pad missing dimensions with exact zeros (grad.hip, kbuild.hip: the pair loops run over DMAX
    dimensions unconditionally), so L, alpha, the log-likelihood, mu and sigma^2 of a 130-point query and every gradient entry
    are bitwise the same; SE-ARD's new length-scale entry is exactly 0.  No tolerance: a mismatch means two instantiations
    round differently (e.g. an fma contracted in one and not the other)."""
    pb = HD.problem(kind, HD.INVARIANCE_N, D)
    pb1 = HD.with_constant_column(pb)
    Xq = HD.query_points(pb, 130)
    Xq1 = np.hstack([Xq, np.full((130, 1), pb1.X[0, -1])])
    a, b = _everything(engine_lib, pb, Xq), _everything(engine_lib, pb1, Xq1)
    for key in ("L", "alpha", "kta", "var"):
        assert np.array_equal(a[key], b[key]), key
    assert a["ll"] == b["ll"]
    gb = b["grad"]
    if kind == O.SE_ARD:  # [ell_1 .. ell_D, ell_new | sigma_f | noise]
        assert gb[D] == 0.0
        gb = np.delete(gb, D)
    assert np.array_equal(a["grad"], gb)


# --------------------------------------------------------------------------------------- 3. full path against the oracle
def _blocks(kind, D, k, n):
    """The parameter vector by block: [ell | Lambda columns | sigma_f | (noise)] (SE-ARD), [l | sigma_f | (noise)]."""
    if kind != O.SE_ARD:
        return [slice(0, 1), slice(1, 2)] + ([slice(2, 3)] if n > 2 else [])
    nt = D + D * k + 1
    out = [slice(0, D)] + [slice(D * (j + 1), D * (j + 2)) for j in range(k)] + [slice(nt - 1, nt)]
    return out + ([slice(nt, nt + 1)] if n > nt else [])


def _check_grad(gg, go):
    assert relerr_norm(gg, go) < PC.TOL_GRAD
    err = HD.grad_component_err(gg, go)
    assert np.max(err) < PC.TOL_GRAD, (int(np.argmax(err)), float(np.max(err)))


def _check_queries(g, o, Xq, mean, noise):
    kg, vg = g.query_batch(Xq)
    ko, vo = o.query_batch(Xq)
    mug, s2g = O.finish_query(kg, vg, mean, noise)
    muo, s2o = O.finish_query(ko, vo, mean, noise)
    assert relerr(mug, muo, floor=1e-3) < PC.TOL_MU
    assert relerr(s2g, s2o) < PC.TOL_VAR


@pytest.mark.parametrize("case", HD.FULL_CASES, ids=lambda c: c[0])
def test_gpu_full_path_vs_oracle(engine_lib, oracle_lib, case):
    """Every entry point at kp.D > 16 against the C oracle on the same inputs; the case id names the instantiation it exists for
    (tests/high_dim.py: FULL_CASES): K, L (and L L^T against K), alpha, log-likelihood, K^-1; the gradient with optimize_noise
    off and on — in norm, per block of the parameter vector and per component (floor 1e-3 ||g||_inf); LOO and its gradient
    (N <= 300); mu / sigma^2 of <= 8 points (the one-workgroup small path, N <= 256) and of 130; add_sample; a clone answering
    bitwise like its source; the hyper-parameter objective at a second theta; no data-flow retries."""
    _, kind, N, D, k, P, seed = case
    pb = HD.full_problem(kind, N, D, k, P, seed)
    nt = HD.n_theta(kind, D, k)
    assert pb.theta.size == nt
    g = new_gp(engine_lib, kind, pb.X, pb.obs_mean, pb.theta, pb.noise)
    o = new_gp(oracle_lib, kind, pb.X, pb.obs_mean, pb.theta, pb.noise)
    Kg, Ko = g.get_K(), o.get_K()
    # (with Lambda the device sums squares of the projections Lambda^T x_i - Lambda^T x_j, the oracle forms d^T M d: the
    #  cancellation differs — test_gpu_parity.py::test_gpu_se_ard_lambda_vs_oracle's 1e-11)
    assert relerr(Kg, Ko, floor=1e-30) < (HD.K_BAR if k == 0 else 1e-11)
    assert g.compute() == 0 and o.compute() == 0
    Lg, Lo = g.get_L(), o.get_L()
    assert np.all(np.triu(Lg, 1) == 0.0)
    assert np.max(np.abs(Lg - Lo)) < 1e-10 * np.max(np.abs(Lo))
    # the factorised K (k_build_wide / generated tiles) against get_K's (the oracle's without Lambda), entry by entry
    assert _llt_err(Lg, Ko if k == 0 else Kg) < HD.LLT_BAR
    del Kg, Ko
    assert relerr_norm(g.get_alpha(), o.get_alpha()) < 1e-7
    llg, llo = g.log_lik(), o.log_lik()
    assert abs(llg - llo) <= PC.TOL_LL * max(1.0, abs(llo))
    assert relerr_norm(g.get_Kinv(), o.get_Kinv()) < 1e-8
    for on in (False, True):
        gg, go = g.log_lik_grad(on), o.log_lik_grad(on)
        assert gg.size == nt + on
        _check_grad(gg, go)
        for sl in _blocks(kind, D, k, gg.size):  # (a small block cannot hide behind a large one)
            assert relerr_norm(gg[sl], go[sl]) < 10 * PC.TOL_GRAD, sl
    assert abs(g.log_loo_cv() - o.log_loo_cv()) <= 1e-9 * max(1.0, abs(o.log_loo_cv()))
    if N <= 300:  # (the oracle's LOO gradient is T dense N^3 products)
        assert relerr_norm(g.log_loo_cv_grad(True), o.log_loo_cv_grad(True)) < PC.TOL_GRAD
        assert relerr_norm(g.log_lik_grad(True), o.log_lik_grad(True)) < PC.TOL_GRAD  # (the LOO path reuses the L^-1 scratch)
    Xq = HD.query_points(pb, 130)
    if N <= 256:
        for m in (1, 8):
            _check_queries(g, o, Xq[:m], pb.mean, pb.noise)
    _check_queries(g, o, Xq, pb.mean, pb.noise)
    # incremental update (gp.hpp:573-603), then a clone answering bitwise like its source
    xn = Xq[-1]
    Y2 = np.vstack([pb.Y, np.cos((np.arange(P) + 1) * xn.sum())[None, :]])
    om2, mean2 = O.obs_mean_data(Y2)
    assert g.add_sample(xn, om2) == 0 and o.add_sample(xn, om2) == 0
    assert np.max(np.abs(g.get_L() - o.get_L())) < 1e-9 * np.max(np.abs(Lo))
    assert relerr_norm(g.get_alpha(), o.get_alpha()) < 1e-7
    assert abs(g.log_lik() - o.log_lik()) <= PC.TOL_LL * max(1.0, abs(o.log_lik()))
    if N + 1 <= 256:
        _check_queries(g, o, Xq[:5], mean2, pb.noise)
    _check_queries(g, o, Xq, mean2, pb.noise)
    c = g.clone()
    kc, vc = c.query_batch(Xq)
    k2, v2 = g.query_batch(Xq)
    assert np.array_equal(kc, k2) and np.array_equal(vc, v2)
    assert c.log_lik() == g.log_lik()
    c.close()
    # the objective at a second theta (kernel_lf_opt.hpp:77-92), the noise as a parameter
    th2 = pb.theta + np.random.default_rng(N + D).uniform(-0.1, 0.1, size=nt)
    lg, gg, info = g.hp_objective(kind, th2, 1.5 * pb.noise, optimize_noise=True, want_grad=True)
    lo, go, _ = o.hp_objective(kind, th2, 1.5 * pb.noise, optimize_noise=True, want_grad=True)
    assert info == 0 and abs(lg - lo) <= PC.TOL_LL * max(1.0, abs(lo))
    assert gg.size == nt + 1
    _check_grad(gg, go)
    assert g.flow_retries() == 0
    g.close()
    o.close()


def test_gpu_add_sample_across_256_and_capacity_growth(engine_lib, oracle_lib):
    """add_sample from 250 to 270 samples with Din = 20, k = 2 (kp.D = 22: k_build<32> cross kernels): the small path below 256
    samples, the general one above, and one growth of the device buffers (grow_dev copies the projection rows of Lambda too);
    L, alpha, log-likelihood and queries against the oracle doing the same, and against a fresh compute() at 270."""
    kind, n0, n1, D, k = HD.GROWTH
    pb = HD.growth_problem()
    om0, _ = O.obs_mean_data(pb.Y[:n0])
    g = new_gp(engine_lib, kind, pb.X[:n0], om0, pb.theta, pb.noise)
    o = new_gp(oracle_lib, kind, pb.X[:n0], om0, pb.theta, pb.noise)
    assert g.compute() == 0 and o.compute() == 0
    Xq = HD.query_points(pb, 8)
    for n in range(n0, n1):
        om, mean = O.obs_mean_data(pb.Y[:n + 1])
        assert g.add_sample(pb.X[n], om) == 0 and o.add_sample(pb.X[n], om) == 0
        if n + 1 in (255, 256, 257, n1):
            Lo = o.get_L()
            assert np.max(np.abs(g.get_L() - Lo)) < 1e-9 * np.max(np.abs(Lo)), n + 1
            assert relerr_norm(g.get_alpha(), o.get_alpha()) < 1e-7, n + 1
            assert abs(g.log_lik() - o.log_lik()) <= PC.TOL_LL * max(1.0, abs(o.log_lik())), n + 1
            _check_queries(g, o, Xq, mean, pb.noise)
    om, _ = O.obs_mean_data(pb.Y)
    f = new_gp(oracle_lib, kind, pb.X, om, pb.theta, pb.noise)
    assert f.compute() == 0
    assert np.max(np.abs(g.get_L() - f.get_L())) < 1e-9 * np.max(np.abs(f.get_L()))
    assert g.nb_samples() == n1 and g.flow_retries() == 0
    for h in (g, o, f):
        h.close()


# ---------------------------------------------------------------------------------------------------------- 4. batched
@pytest.mark.parametrize("case", HD.BATCH_CASES, ids=lambda c: c[0])
def test_gpu_batch_high_dim(engine_lib, oracle_lib, case):
    """gpe_batch_compute and gpe_batch_hp_objective at D = 20 (ragged N = 700: the members' K from k_build_wide<..., 32, true>)
    and D = 40 (N = 640 = 10 x 64, G = 5: the batched data-flow launch generates the tiles, t0 = 0 at g = G): every member
    against a single handle (log-likelihood 1e-11, gradient 1e-9) and against the oracle (test_gpu_configs.py::
    test_gpu_batch_hp_objective_vs_single_and_oracle's bars), bitwise reproducible."""
    _, kind, N, D, G = case
    assert HD.plan(N, 1, G)["t0"] == 0
    pbs = [HD.batch_problem(kind, N, D, q) for q in range(G)]
    hs = [new_gp(engine_lib, kind, pb.X, pb.obs_mean, pb.theta, pb.noise) for pb in pbs]
    assert _capi.batch_compute(hs) == [0] * G
    ll = _capi.batch_log_lik(hs)
    nt = HD.n_theta(kind, D)
    th = np.array([pb.theta + 0.05 * (q - G // 2) for q, pb in enumerate(pbs)])
    nz = np.array([pb.noise * (1.0 + 0.2 * q) for q, pb in enumerate(pbs)])
    lik, grad, st = _capi.batch_hp_objective(hs, kind, th, nz, optimize_noise=True, want_grad=True)
    lik2, grad2, st2 = _capi.batch_hp_objective(hs, kind, th, nz, optimize_noise=True, want_grad=True)
    assert st == [0] * G and st2 == [0] * G and np.array_equal(lik, lik2) and np.array_equal(grad, grad2)
    assert grad.shape == (G, nt + 1)
    for q in sorted({0, G // 2, G - 1}):
        pb = pbs[q]
        s = new_gp(engine_lib, kind, pb.X, pb.obs_mean, pb.theta, pb.noise)
        o = new_gp(oracle_lib, kind, pb.X, pb.obs_mean, pb.theta, pb.noise)
        assert s.compute() == 0 and o.compute() == 0
        assert abs(ll[q] - s.log_lik()) <= 1e-11 * abs(s.log_lik())
        assert abs(ll[q] - o.log_lik()) <= PC.TOL_LL * abs(o.log_lik())
        l1, g1, info = s.hp_objective(kind, th[q], nz[q], optimize_noise=True, want_grad=True)
        assert info == 0 and abs(lik[q] - l1) <= 1e-11 * abs(l1) and relerr_norm(grad[q], g1) < 1e-9
        lo, go, _ = o.hp_objective(kind, th[q], nz[q], optimize_noise=True, want_grad=True)
        assert abs(lik[q] - lo) <= PC.TOL_LL * abs(lo)
        _check_grad(grad[q], go)
        assert relerr_norm(hs[q].get_Kinv(), o.get_Kinv()) < 1e-8
        s.close()
        o.close()
    assert all(h.flow_retries() == 0 for h in hs)
    for h in hs:
        h.close()


# ---------------------------------------------------------------------------------------------------------- 5. sparsify
@pytest.mark.parametrize("D", [17, 33, 64])
def test_gpu_sparsify_high_dim_vs_oracle(engine_lib, oracle_lib, D):
    """SparsifiedGP::_sparsify at k_row_density<32> (D = 17), <64> (33, and 64: the top of the accepted range) against the
    oracle, on test_gpu_parity.py::test_gpu_sparsify_vs_oracle's clustered inputs: the same samples kept."""
    N, mp = 300, 120
    rng = np.random.default_rng(7 * N + D)
    X = rng.uniform(0, 1, size=(N, D))
    X[: N // 4] = 0.3 + 0.02 * rng.normal(size=(N // 4, D))
    kg = _capi.sparsify(engine_lib, X, mp)
    ko = _capi.sparsify(oracle_lib, X, mp)
    assert len(kg) == mp and np.array_equal(kg, ko)


def test_gpu_sparsify_argument_limits(engine_lib):
    """D = 65 and max_points <= D (the D nearest neighbours must exist) are argument errors; nothing is launched."""
    rng = np.random.default_rng(65)
    with pytest.raises(_capi.EngineError):
        _capi.sparsify(engine_lib, rng.uniform(0, 1, size=(100, 65)), 80)
    for D, mp in ((17, 17), (33, 20), (64, 64)):
        with pytest.raises(_capi.EngineError):
            _capi.sparsify(engine_lib, rng.uniform(0, 1, size=(100, D)), mp)


# ------------------------------------------------------------------------------------------------------------ 6. limits
def test_gpu_dimension_limits(engine_lib):
    """Host-side argument checks of engine.hip (nothing is launched): D <= GPE_MAX_THETA - 2 = 62 inputs (set_data, add_sample on
    an empty handle); n_theta <= GPE_MAX_THETA = 64 (set_kernel); k <= max_lam(Din) Lambda columns (lam_columns, at set_kernel
    or compute: the test accepts either, as test_gpu_parity.py::test_gpu_se_ard_parameter_count does)."""
    rng = np.random.default_rng(63)
    om = rng.normal(size=(20, 1))
    h = _capi.Handle(engine_lib)
    with pytest.raises(_capi.EngineError):
        h.set_data(rng.uniform(0, 1, size=(20, 63)), om)
    h.close()
    e = _capi.Handle(engine_lib)
    e.set_kernel(O.MATERN52, np.zeros(2), 0.01)
    with pytest.raises(_capi.EngineError):
        e.add_sample(rng.uniform(0, 1, size=63), om[:1])
    e.close()
    for Din, k in ((21, 3), (32, 1)):  # 85 and 65 parameters
        s = new_gp(engine_lib, O.MATERN52, rng.uniform(0, 1, size=(20, Din)), om, np.zeros(2), 0.01)
        with pytest.raises(_capi.EngineError):
            s.set_kernel(O.SE_ARD, np.zeros(HD.n_theta(O.SE_ARD, Din, k)), 0.01)
        s.close()
    s = new_gp(engine_lib, O.MATERN52, rng.uniform(0, 1, size=(20, 7)), om, np.zeros(2), 0.01)
    try:  # 64 parameters pass set_kernel's count, but k = 8 > Din
        s.set_kernel(O.SE_ARD, np.zeros(HD.n_theta(O.SE_ARD, 7, 8)), 0.01)
        rc = s.compute()
    except _capi.EngineError:
        rc = -1
    assert rc != 0
    s.close()
    for Din, k in ((62, 0), (21, 2)):  # the largest accepted (test_gpu_full_path_vs_oracle computes with both)
        s = new_gp(engine_lib, O.SE_ARD, rng.uniform(0, 1, size=(20, Din)), om, np.zeros(HD.n_theta(O.SE_ARD, Din, k)), 0.01)
        s.close()


# ------------------------------------------------------------------------------------------------- the mpmath goldens
@pytest.mark.parametrize("path", HD.high_dim_goldens(), ids=lambda p: p.stem)
def test_gpu_vs_mpmath_golden_grad_per_component(engine_lib, path):
    """The high-dimensional goldens' gradients per component (test_gpu_parity.py::test_gpu_vs_mpmath_golden checks the rest)."""
    HD.check_golden_grad_per_component(engine_lib, path)
