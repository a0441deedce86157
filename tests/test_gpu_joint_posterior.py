"""The joint posterior over a point batch on the device (include/gpe_joint.h): covariance, draws, arg-max, and the C++ drop-in.

The checker is never the engine: Sigma_ref, mu_ref and the draws come from the CPU oracle's factor and alpha and numpy / LAPACK
(two such routes, Cholesky and LU, agree to 1.2e-14 on these inputs, so the reference uses a millionth of the 1e-8 bar).
Inputs: X and V uniform in [0, 1]^D, sigma_f = 1 (so the bars are absolute), noise 0.01."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.linalg as sla

from limbo_amd import _capi
from oracle import np_oracle as O
from tests.test_joint_posterior import reference, run_driver

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NOISE = 0.01
ELL6 = np.log([0.3, 0.45, 0.6, 0.75, 0.9, 1.0, 1.0])  # SE-ARD, D = 6: length scales 0.3 .. 1.0, sigma_f = 1
# ... for 2048 points: with ELL6 their covariance has cond(Sigma + 1e-8 I) = 5.5e5 (computed on the CPU from the oracle's factor when
# this test was written), beyond the 1e5 under which draws are comparable at 1e-8; with these it is 4.7e4
ELL6_DENSE = np.log([0.3, 0.35, 0.4, 0.5, 0.7, 1.0, 1.0])

# name: (kind, N, M, D, P, log theta)
CASES = {
    "se_ard_2048x1024": (O.SE_ARD, 2048, 1024, 6, 1, ELL6),
    "matern52_2048x1024_p2": (O.MATERN52, 2048, 1024, 6, 2, np.log([0.7, 1.0])),
    "se_ard_4096x2048_p2": (O.SE_ARD, 4096, 2048, 6, 2, ELL6_DENSE),
    "matern52_1700x700": (O.MATERN52, 1700, 700, 6, 1, np.log([0.7, 1.0])),
    "se_ard_300x65_p2": (O.SE_ARD, 300, 65, 6, 2, ELL6),
    "se_ard_lambda1_4096x129": (O.SE_ARD, 4096, 129, 5, 1, np.concatenate([np.log(np.linspace(0.3, 1.0, 5)), [0.4, -0.3, 0.2, 0.5, -0.1], [0.0]])),
    "se_ard_d20_1700x700": (O.SE_ARD, 1700, 700, 20, 1, np.concatenate([np.log(np.linspace(0.3, 1.0, 20)), [0.0]])),
}
SEEDS = {name: 11 + i for i, name in enumerate(CASES)}
_cache = {}


def problem(name, oracle_lib):
    """inputs and the reference of a case (once per session: the oracle's factorisation is seconds of single-core work)"""
    if name in _cache:
        return _cache[name]
    kind, N, M, D, P, th = CASES[name]
    rng = np.random.default_rng(SEEDS[name])
    X, V = rng.random((N, D)), rng.random((M, D))
    Y = np.stack([np.sin(3.0 * X @ rng.random(D)) + 0.1 * rng.standard_normal(N) for _ in range(P)], axis=1)
    om = Y - Y.mean(axis=0)
    o = _capi.Handle(oracle_lib)
    o.set_data(X, om)
    o.set_kernel(kind, th, NOISE)
    assert o.compute() == 0
    L, al = o.get_L(), o.get_alpha()
    o.close()
    Ks = O.kernel_cross(kind, X, V, th)
    Zs = sla.solve_triangular(L, Ks, lower=True)
    pr = dict(kind=kind, N=N, M=M, D=D, P=P, th=th, X=X, V=V, om=om, Sig=O.kernel_cross(kind, V, V, th) - Zs.T @ Zs, kta=Ks.T @ al,
              Z=rng.standard_normal((M, 16, P)), mq=rng.standard_normal((M, P)))
    _cache[name] = pr
    return pr


def model(engine_lib, pr):
    h = _capi.Handle(engine_lib)
    h.set_data(pr["X"], pr["om"])
    h.set_kernel(pr["kind"], pr["th"], NOISE)
    assert h.compute() == 0
    return h


def check_cov_and_kta(h, pr, jitter=0.0):
    """the checks of one covariance path on a computed handle; returns (kta, cov)"""
    M = pr["M"]
    k0, v0 = h.query_batch(pr["V"])
    kta, cov = h.joint_query(pr["V"], jitter)
    d_cov = np.max(np.abs(cov - pr["Sig"] - jitter * np.eye(M)))
    d_kta = np.max(np.abs(kta - pr["kta"]))
    d_var = np.max(np.abs(np.diag(cov) - jitter - v0))
    print(f"max|Sigma - ref| = {d_cov:.3e}, max|kta - ref| = {d_kta:.3e}, max|diag - var| = {d_var:.3e}")
    assert d_cov <= 1e-8
    assert d_kta <= 1e-8 * max(1.0, np.max(np.abs(pr["kta"])))
    assert np.array_equal(cov, cov.T), "cov is exactly symmetric"
    assert d_var <= 1e-10
    assert np.array_equal(kta, k0), "kta is bitwise gpe_query_batch's"
    kta1, none = h.joint_query(pr["V"], jitter, want_cov=False)
    none2, cov1 = h.joint_query(pr["V"], jitter, want_mu=False)
    assert none is None and none2 is None and np.array_equal(kta1, kta) and np.array_equal(cov1, cov)
    return kta, cov


@pytest.mark.parametrize("name", list(CASES))
def test_covariance_and_kta(engine_lib, oracle_lib, name):
    pr = problem(name, oracle_lib)
    h = model(engine_lib, pr)
    assert h.joint_max_points() >= pr["M"]
    check_cov_and_kta(h, pr, 0.0)
    check_cov_and_kta(h, pr, 1e-6)
    assert h.flow_retries() == 0 and h.handover_reruns() == 0
    h.close()


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from limbo_amd import _capi
from tests import test_gpu_joint_posterior as T
z = np.load(sys.argv[2])
pr = {k: (z[k].item() if z[k].ndim == 0 else z[k]) for k in z.files}
h = T.model(_capi.load_engine(), pr)
kta, cov = T.check_cov_and_kta(h, pr, 1e-6)
assert h.flow_retries() == 0 and h.handover_reruns() == 0
np.save(sys.argv[3], cov)
print("child ok")
"""


@pytest.mark.parametrize("name", list(CASES))
def test_both_covariance_paths(tmp_path, engine_lib, oracle_lib, name):
    """GPE_JOINT_SPLITK=0 (a child process: the switch is read once): the composed path — kernel-matrix build on V, the
    triangular matrix-core update with k = N, the mirror — passes the same checks, and the default path agrees with it to 1e-12"""
    pr = problem(name, oracle_lib)
    np.savez(tmp_path / "pr.npz", **pr)
    r = subprocess.run([sys.executable, "-c", _CHILD, str(ROOT), str(tmp_path / "pr.npz"), str(tmp_path / "cov.npy")],
                       env=dict(os.environ, GPE_JOINT_SPLITK="0"), capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    composed = np.load(tmp_path / "cov.npy")
    h = model(engine_lib, pr)
    _, cov = h.joint_query(pr["V"], 1e-6, want_mu=False)
    h.close()
    d = np.max(np.abs(cov - composed))
    print(f"max|split - composed| = {d:.3e}")
    assert d <= 1e-12


def draw_reference(pr, jitter):
    A = pr["Sig"] + jitter * np.eye(pr["M"])
    # a condition on the INPUTS: the comparison of draws is only meaningful while Sigma + jitter I is well conditioned
    cond = np.linalg.cond(A)
    assert cond <= 1e5, cond
    C = np.linalg.cholesky(A)
    return pr["mq"][:, None, :] + pr["kta"][:, None, :] + np.einsum("mj,jsp->msp", C, pr["Z"])


@pytest.mark.parametrize("jitter", [1e-8, 1e-6, NOISE])
@pytest.mark.parametrize("name", list(CASES))
def test_draws_and_argmax(engine_lib, oracle_lib, name, jitter):
    pr = problem(name, oracle_lib)
    Fr = draw_reference(pr, jitter)
    h = model(engine_lib, pr)
    rc, F, am, fm = h.joint_draws(pr["V"], pr["Z"], jitter, mean_q=pr["mq"])
    assert rc == 0
    d = np.max(np.abs(F - Fr))
    print(f"max|F - ref| = {d:.3e}")
    assert d <= 1e-8
    # arg-max per draw, wherever the reference's two largest values are further apart than 1e-6
    top2 = np.sort(Fr, axis=0)[-2:]
    clear = (top2[1] - top2[0]) > 1e-6
    assert (~clear).sum() <= 1, "at most one draw of a case may be left out as a near-tie"
    assert np.array_equal(am[clear], Fr.argmax(axis=0)[clear])
    assert np.max(np.abs(fm - Fr.max(axis=0))) <= 1e-8
    assert np.array_equal(fm, F.max(axis=0)) and np.array_equal(am, F.argmax(axis=0))
    rc2, F2, am2, fm2 = h.joint_draws(pr["V"], pr["Z"], jitter, mean_q=pr["mq"], want_F=False)
    assert rc2 == 0 and F2 is None and np.array_equal(am2, am) and np.array_equal(fm2, fm), "with F == NULL the arg-max is bitwise the same"
    # mean_q == NULL is zero
    rc3, F3, _, _ = h.joint_draws(pr["V"], pr["Z"], jitter, want_argmax=False)
    assert rc3 == 0 and np.max(np.abs(F3 + pr["mq"][:, None, :] - F)) <= 1e-12
    assert h.flow_retries() == 0 and h.handover_reruns() == 0
    h.close()


@pytest.mark.parametrize("jitter", [1e-8, 1e-6, NOISE])
def test_factor_recovered_column_by_column(engine_lib, oracle_lib, jitter):
    """independent of conditioning: Z = e_j recovers column j of C, and C C^T must be Sigma_ref + jitter I"""
    pr = problem("se_ard_300x65_p2", oracle_lib)
    M, P = pr["M"], pr["P"]
    h = model(engine_lib, pr)
    Z = np.zeros((M, M, P))
    Z[:, :, 0] = np.eye(M)
    rc, F, _, _ = h.joint_draws(pr["V"], Z, jitter, want_argmax=False)
    assert rc == 0
    kta, _ = h.joint_query(pr["V"], jitter, want_cov=False)
    C = F[:, :, 0] - kta[:, 0][:, None]
    assert np.max(np.abs(np.triu(C, 1))) <= 1e-13 * np.max(np.abs(C)), "C is lower triangular"
    d = np.max(np.abs(C @ C.T - pr["Sig"] - jitter * np.eye(M)))
    print(f"max|C C^T - (Sigma + jitter I)| = {d:.3e}")
    assert d <= 1e-10
    assert np.array_equal(F[:, :, 1], np.repeat(kta[:, 1][:, None], M, axis=1)), "Z = 0 for the second output: its draws are the mean"
    h.close()


def test_argmax_tie_takes_the_lowest_index(engine_lib, oracle_lib):
    pr = problem("se_ard_300x65_p2", oracle_lib)
    h = model(engine_lib, pr)
    V = np.repeat(pr["V"][:1], 2, axis=0)  # two identical rows as the only points
    rc, F, am, fm = h.joint_draws(V, np.zeros((2, 3, pr["P"])), NOISE, mean_q=np.zeros((2, pr["P"])))
    assert rc == 0 and np.array_equal(F[0], F[1])
    assert np.array_equal(am, np.zeros_like(am)) and np.array_equal(fm, F[0])
    h.close()


def test_determinism_and_constness(engine_lib, oracle_lib):
    pr = problem("se_ard_2048x1024", oracle_lib)
    h = model(engine_lib, pr)
    ll0, ep0 = h.log_lik(), h.epoch()
    k0, v0 = h.query_batch(pr["V"])
    a = h.joint_query(pr["V"], 1e-6)
    da = h.joint_draws(pr["V"], pr["Z"], 1e-6, mean_q=pr["mq"])
    b = h.joint_query(pr["V"], 1e-6)
    db = h.joint_draws(pr["V"], pr["Z"], 1e-6, mean_q=pr["mq"])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "two calls are bitwise equal"
    assert da[0] == db[0] == 0 and all(np.array_equal(x, y) for x, y in zip(da[1:], db[1:]))
    # another batch size in between (the scratch context is re-used while M fits, its order changes)
    h.joint_draws(pr["V"][:200], pr["Z"][:200], 1e-6)
    dc = h.joint_draws(pr["V"], pr["Z"], 1e-6, mean_q=pr["mq"])
    assert all(np.array_equal(x, y) for x, y in zip(da[1:], dc[1:]))
    # the model is untouched: epoch, log-likelihood and the marginal queries are bitwise what they were
    assert h.epoch() == ep0 and h.log_lik() == ll0
    k1, v1 = h.query_batch(pr["V"])
    assert np.array_equal(k0, k1) and np.array_equal(v0, v1)
    kp, vp = h.query_batch(pr["V"][:3])  # (the few-point path reads the diagonal-block inverses of L)
    c = h.clone()
    kc, vc = c.query_batch(pr["V"][:3])
    assert np.array_equal(kp, kc) and np.array_equal(vp, vc)
    c.close()
    assert h.flow_retries() == 0 and h.handover_reruns() == 0
    h.close()


def test_status_and_limits(engine_lib, oracle_lib):
    pr = problem("se_ard_300x65_p2", oracle_lib)
    V, Z, P = pr["V"], pr["Z"], pr["P"]
    lib = engine_lib
    h = _capi.Handle(lib)
    h.set_data(pr["X"], pr["om"])
    h.set_kernel(pr["kind"], pr["th"], NOISE)
    raw_q, raw_d = lib.fn("joint_query"), lib.fn("joint_draws")
    Vc = np.ascontiguousarray(V)
    cov = np.zeros((65, 65), order="F")
    Zf = np.asfortranarray(Z.reshape(65, -1, order="F"))
    F = np.zeros_like(Zf, order="F")
    args_q = lambda M, jit: raw_q(h._h, _capi._d(Vc), M, jit, None, _capi._d(cov), 65)
    args_d = lambda M, jit, S: raw_d(h._h, _capi._d(Vc), M, jit, None, _capi._d(Zf), S, _capi._d(F), None, None)
    assert args_q(65, 0.0) == -2 and args_d(65, 0.0, 16) == -2, "GPE_ERR_STATE before compute"
    assert h.compute() == 0
    for bad in (-1e-9, float("nan"), float("inf")):
        assert args_q(65, bad) == -1 and args_d(65, bad, 16) == -1
    assert args_q(-1, 0.0) == -1 and args_d(-1, 0.0, 16) == -1 and args_d(65, 0.0, -1) == -1
    assert args_q(0, 0.0) == 0 and args_d(0, 0.0, 16) == 0, "M = 0 is a no-op"
    cap = h.joint_max_points()
    assert cap >= 65
    big = np.zeros((cap + 1, pr["D"]))
    assert raw_q(h._h, _capi._d(big), cap + 1, 0.0, None, None, cap + 1) == -1, "M above the cap"
    assert args_q(65, 0.0) == 0 and args_d(65, 1e-6, 16) == 0
    # two identical points and no jitter: Sigma is singular and rounding decides whether the second pivot comes out <= 0 — the
    # status is 0 or that pivot's 1-based index, never an error, and Sigma and kta are valid either way
    V2 = np.ascontiguousarray(np.repeat(V[:1], 2, axis=0))
    rc = raw_d(h._h, _capi._d(V2), 2, 0.0, None, _capi._d(np.zeros((2, P), order="F")), 1, None, None, None)
    assert rc in (0, 2), rc
    kta2, cov2 = h.joint_query(V2, 0.0)
    assert np.all(np.isfinite(cov2)) and cov2[0, 0] == cov2[1, 1] == cov2[0, 1] and np.array_equal(kta2[0], kta2[1])
    h.close()
    # the cap at N = 16 384 (no factorisation needed to ask)
    g = _capi.Handle(lib)
    g.set_data(np.random.default_rng(0).random((16384, 2)), np.zeros((16384, 1)))
    assert g.joint_max_points() >= 8192
    g.close()
    # kernels without device code are served by the drop-in's host route
    k = _capi.Handle(lib)
    Xs = pr["X"][:300]
    k.set_data(Xs, pr["om"][:300])
    k.set_kernel(_capi.KERNEL_HOST_K, np.zeros(0), NOISE)
    k.set_K_host(O.kernel_matrix(pr["kind"], Xs, pr["th"], NOISE))
    assert k.compute() == 0
    assert raw_q(k._h, _capi._d(Vc), 65, 0.0, None, _capi._d(cov), 65) == -5, "GPE_ERR_UNSUPPORTED for GPE_KERNEL_HOST_K"
    k.close()


# ------------------------------------------------------------------------------------------------ the C++ drop-in on the device
def _dropin_problem(kind, mean, P, n, M, seed):
    D = 3 if kind == 0 else 2
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, size=(n, D))
    Y = np.stack([np.cos((p + 1.5) * X.sum(axis=1)) + 0.3 * X[:, 0] for p in range(P)], axis=1) + 0.05 * rng.normal(size=(n, P))
    return X, Y, rng.uniform(0, 1, size=(M, D))


@pytest.mark.parametrize("kind,mean,P,n", [(0, 0, 1, 600), (1, 2, 2, 2000), (0, 2, 2, 2000), (1, 0, 1, 600)])
def test_dropin_on_the_device(tmp_path, oracle_lib, kind, mean, P, n):
    """models above Params::gpu::min_n_for_gpu: query_joint and sample run through gpe_joint_query / gpe_joint_draws"""
    M, S, q, jitter = 40, 5, 4, 1e-6
    X, Y, Q = _dropin_problem(kind, mean, P, n, M, 31 * n + kind)
    Z = np.random.default_rng(n).standard_normal((M, S, P))
    got = run_driver(tmp_path, kind, mean, X, Y, Q, Z, q, jitter, 7)
    assert got["host_resident"][0] == 0
    mu, Sig, F = reference(oracle_lib, kind, mean, X, Y, Q, Z, jitter)
    assert np.max(np.abs(got["mu"] - mu)) <= 1e-8 * max(1.0, np.max(np.abs(mu)))
    assert np.max(np.abs(got["cov"] - Sig)) <= 1e-8
    assert np.array_equal(got["cov"], got["cov"].T)
    assert np.linalg.cond(Sig) <= 1e5
    assert np.max(np.abs(got["F"] - F)) <= 1e-8
    var = got["sigma"] - NOISE
    live = var > np.finfo(float).eps
    assert np.max(np.abs((np.diag(got["cov"]) - jitter - var)[live])) <= 1e-10
    assert list(got["seed_repeat"]) == [1, 1]
    assert len(got["thompson"]) == q and np.array_equal(got["thompson"], got["thompson_host"])


def test_thompson_batch_on_the_device(tmp_path):
    """q = 8 proposals from 2000 candidates: the device arg-max (the draws never leave the device) equals the host arg-max over
    sample() with the same seed"""
    X, Y, Q = _dropin_problem(0, 0, 1, 2000, 2000, 5)
    got = run_driver(tmp_path, 0, 0, X, Y, Q, np.zeros((2000, 0, 1)), 8, 1e-6, 12345, brief=True)
    assert got["host_resident"][0] == 0
    assert len(got["thompson"]) == 8 and np.array_equal(got["thompson"], got["thompson_host"])
    assert len(set(got["thompson"].tolist())) > 1, "independent draws do not all propose the same candidate"


@pytest.mark.parametrize("kind,mean,P,n", [(0, 0, 1, 1), (0, 0, 1, 2), (1, 2, 2, 40), (0, 0, 2, 200), (1, 0, 1, 200)])
def test_dropin_small_models_forced_onto_the_device(tmp_path, oracle_lib, kind, mean, P, n):
    """LIMBO_AMD_MIN_N_FOR_GPU=0: the small models of the CPU test through the engine (fewer samples than one outer panel: the
    N x M layout and the composed covariance path)"""
    M, S, q, jitter = 12, 5, 4, 1e-6
    X, Y, Q = _dropin_problem(kind, mean, P, n, M, 1000 * kind + 100 * mean + 10 * P + n)
    Z = np.random.default_rng(n).standard_normal((M, S, P))
    got = run_driver(tmp_path, kind, mean, X, Y, Q, Z, q, jitter, 7, env={"LIMBO_AMD_MIN_N_FOR_GPU": "0"})
    assert got["host_resident"][0] == 0
    mu, Sig, F = reference(oracle_lib, kind, mean, X, Y, Q, Z, jitter)
    assert np.max(np.abs(got["mu"] - mu)) <= 1e-8 * max(1.0, np.max(np.abs(mu)))
    assert np.max(np.abs(got["cov"] - Sig)) <= 1e-8
    assert np.array_equal(got["cov"], got["cov"].T)
    assert np.max(np.abs(got["F"] - F)) <= 1e-8
    assert np.array_equal(got["thompson"], got["thompson_host"])


@pytest.mark.parametrize("kind,mean,P,n", [(0, 0, 2, 200), (1, 2, 1, 40)])
def test_dropin_host_model_through_its_device_shadow(tmp_path, oracle_lib, kind, mean, P, n):
    """LIMBO_AMD_HOST_BATCH_CROSSOVER=0: a host-resident model answers the joint calls from its device copy (the host factor and
    alpha uploaded, as for large query_batch() calls)"""
    M, S, q, jitter = 12, 5, 4, 1e-6
    X, Y, Q = _dropin_problem(kind, mean, P, n, M, 77 + n)
    Z = np.random.default_rng(n).standard_normal((M, S, P))
    got = run_driver(tmp_path, kind, mean, X, Y, Q, Z, q, jitter, 7, env={"LIMBO_AMD_HOST_BATCH_CROSSOVER": "0"})
    assert got["host_resident"][0] == 1
    mu, Sig, F = reference(oracle_lib, kind, mean, X, Y, Q, Z, jitter)
    assert np.max(np.abs(got["mu"] - mu)) <= 1e-8 * max(1.0, np.max(np.abs(mu)))
    assert np.max(np.abs(got["cov"] - Sig)) <= 1e-8
    assert np.max(np.abs(got["F"] - F)) <= 1e-8
    assert np.array_equal(got["thompson"], got["thompson_host"])
