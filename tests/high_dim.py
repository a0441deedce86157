"""Problems above 16 input dimensions (and the same construction below): one builder for tests/test_high_dim_problems.py
(CPU: the preconditions that make the problems sharp), tests/test_gpu_high_dim.py (GPU) and oracle/make_golden.py.

The kernels are compiled once per dimension bucket (DMAX 2 4 6 8 16 32 64; the host picks the bucket from kp.D = input
dimensions + Lambda columns).  A test of a bucket is only as good as its problem: with uniform inputs and unit length scales
K is nearly diagonal at high D (z ~ D / 6 per pair) and a dropped or mis-weighted dimension barely moves L.  So
  * the length scales grow with sqrt(D) and the expected z of a pair is ~3 at every D (k ~ 0.2 sigma_f^2);
  * every dimension carries its own weight: per-dimension log-offsets spread over +-0.7 (SE-ARD: in the length scales;
    isotropic kernels: in the input scale of the column), in a seeded permutation of an even grid so that no two dimensions
    weigh the same;
  * the last dimension carries the heaviest weight (shortest length scale), so that dropping it moves K and the
    log-likelihood by many times the tests' bars.
tests/test_high_dim_problems.py checks these properties for every problem the GPU tests build.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from oracle import np_oracle as O
from tests import parity_checks as PC
from tests.util import golden_files, load, new_gp

KINDS = (O.SE_ARD, O.MATERN52, O.MATERN32, O.EXP)
KIND_NAMES = {O.SE_ARD: "se_ard", O.MATERN52: "matern52", O.MATERN32: "matern32", O.EXP: "exp"}
Z_MEAN = 3.0  # expected z = sum_d ((x_i,d - x_j,d) / ell_d)^2 of a pair of U(0, 1)^D inputs
SPREAD = 0.7  # per-dimension log-offsets in [-SPREAD, SPREAD]
K_BAR = 5e-14  # get_K against the reference K, relative, entry by entry
LLT_BAR = 1e-13  # L L^T of the factorised K against the reference K, entry by entry, relative to max diag K

# the K sweep (test_gpu_high_dim.py::test_gpu_kernel_matrix_sweep): both sides of every bucket edge, the top of the range
SWEEP_D = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 61, 62)
# N = 100: k_build_wide builds all of K (one-launch factorisation not taken, t0 = -1); 320: tiles generated inside k_tail
# (t0 = 0, K never written); 333: generated tiles + a k_build_wide ragged block; 3392: k_build_wide + tall / closing launches
SWEEP_N = (100, 320, 333)
BIG_N, BIG_D = 3392, (6, 20, 62)
BIG_COLS = 256
# bitwise bucket invariance: (D, D + 1) straddle a bucket edge of k_build / k_build_wide / k_grad_tiles, or sit at the top
INVARIANCE_PAIRS = ((2, 3), (4, 5), (6, 7), (8, 9), (16, 17), (32, 33), (61, 62))
INVARIANCE_N = 333


def _seed(*key):
    return int(np.random.SeedSequence([int(v) for v in key]).generate_state(1)[0])


def offsets(rng, D):
    """Per-dimension log-offsets: an even grid over [-SPREAD, SPREAD], seeded order, the LAST dimension at -SPREAD (the
    shortest length scale / widest input scale)."""
    if D == 1:
        return np.array([-SPREAD])
    grid = np.linspace(-SPREAD, SPREAD, D)
    o = np.empty(D)
    o[:-1] = rng.permutation(grid[1:])
    o[-1] = grid[0]
    return o


def problem(kind, N, D, P=1, k=0, seed=0, noise=0.01):
    """A GP problem at D input dimensions (k Lambda columns for SE-ARD).  `seed`: an int, or a numpy Generator to draw from
    (oracle/make_golden.py continues its own stream).  Returns a namespace with X (N x D in [0, 1] times the column scales),
    Y, obs_mean, mean, theta, noise, kind, D, k."""
    rng = seed if isinstance(seed, np.random.Generator) else np.random.default_rng(_seed(kind, N, D, P, k, seed))
    o = offsets(rng, D)
    X = rng.uniform(0, 1, size=(N, D))
    w = np.exp(-2.0 * o)  # weight of each dimension in z
    if kind == O.SE_ARD:
        lam_share = 0.2 if k else 0.0  # the part of z the Lambda projections carry
        c2 = w.sum() / (6.0 * Z_MEAN * (1.0 - lam_share))  # E[(x_i,d - x_j,d)^2] = 1/6
        log_ell = 0.5 * np.log(c2) + o  # ell_d = c exp(o_d): ~ sqrt(D) at fixed z
        lam = rng.uniform(-1.0, 1.0, size=(k, D)) * np.sqrt(3.0 * 6.0 * Z_MEAN * lam_share / (k * D)) if k else np.zeros((0, D))
        theta = np.concatenate([log_ell, lam.reshape(-1), [rng.uniform(-0.2, 0.2)]])
    else:
        X = X * np.exp(-o)  # the isotropic kernels weigh a dimension by its input scale
        l2 = w.sum() / (6.0 * Z_MEAN)
        theta = np.array([0.5 * np.log(l2), rng.uniform(-0.2, 0.2)])
    # observations: smooth in the heavy dimensions (the last one among them) + noise
    s = X @ (w / w.sum() * np.sqrt(D))
    Y = np.stack([np.cos((p + 1) * s) + np.sin(2.0 * X[:, -1] / np.exp(o[-1])) + 0.05 * rng.normal(size=N) for p in range(P)], axis=1)
    om, mean = O.obs_mean_data(Y)
    return SimpleNamespace(kind=kind, X=X, Y=Y, obs_mean=om, mean=mean, theta=theta, noise=float(noise), D=D, k=k, N=N, P=P)


def truncated(pb, D2):
    """The same problem on its first D2 input dimensions: what a kernel that dropped dimensions D2.. would compute."""
    th = pb.theta
    if pb.kind == O.SE_ARD:
        D, k = pb.D, pb.k
        lam = th[D:D + D * k].reshape(k, D)[:, :D2]
        th = np.concatenate([th[:D2], lam.reshape(-1), th[-1:]])
    return SimpleNamespace(**dict(vars(pb), X=pb.X[:, :D2].copy(), theta=th, D=D2))


def with_constant_column(pb, value=0.375):
    """pb with one more input column, constant over the samples (SE-ARD: one more length scale, log-ell 0).  The pair
    differences of that column are exact zeros, so every kernel value, and every gradient entry but the new one, is the
    same number; the new length scale's gradient entry is exactly 0."""
    assert pb.k == 0
    X = np.hstack([pb.X, np.full((pb.N, 1), value)])
    th = np.concatenate([pb.theta[:pb.D], [0.0], pb.theta[pb.D:]]) if pb.kind == O.SE_ARD else pb.theta
    return SimpleNamespace(**dict(vars(pb), X=X, theta=th, D=pb.D + 1))


def n_theta(kind, D, k=0):
    return D + D * k + 1 if kind == O.SE_ARD else 2


def query_points(pb, M, seed=1):
    """M query points inside the inputs' box; the first three ON training points (sigma^2 cancellation / clamp path)."""
    rng = np.random.default_rng(_seed(pb.kind, pb.N, pb.D, pb.k, M, seed))
    hi = pb.X.max(axis=0)
    Xq = rng.uniform(0, 1, size=(M, pb.D)) * hi
    Xq[:min(3, M)] = pb.X[:min(3, M)]
    return Xq


def kernel_columns(kind, X, theta, noise, cols):
    """K[:, cols] of kernel_matrix (np_oracle) without forming K: rows in chunks."""
    cols = np.asarray(cols)
    out = np.empty((X.shape[0], cols.size))
    for r0 in range(0, X.shape[0], 512):
        out[r0:r0 + 512] = O.kernel_cross(kind, X[r0:r0 + 512], X[cols], theta)
    hit = np.nonzero(cols[None, :] == np.arange(X.shape[0])[:, None])
    out[hit] += noise + 1e-8
    return out


def sweep_cases():
    return [(kind, N, D) for kind in KINDS for D in SWEEP_D for N in SWEEP_N]


def big_cases():
    return [(kind, BIG_N, D) for kind in KINDS for D in BIG_D]


def big_columns(N):
    return np.sort(np.random.default_rng(_seed(N, BIG_COLS)).choice(N, size=BIG_COLS, replace=False))


# the full path against the C oracle (test_gpu_high_dim.py::test_gpu_full_path_vs_oracle): what each case exists for.  The seeds
# are the first ones whose gradient components are pairwise >= 1e-3 apart (test_high_dim_problems.py)
#          id                                                          kind        N     Din k  P  seed
FULL_CASES = [("se_ard_n333_d17_p1-build32_grad32_pm1_generated_tiles_ragged", O.SE_ARD, 333, 17, 0, 1, 3),
              ("se_ard_n700_d20_p2-grad32_pm8_large_query", O.SE_ARD, 700, 20, 0, 2, 3),
              ("se_ard_n1100_d33_p1-build64_grad64_pm1", O.SE_ARD, 1100, 33, 0, 1, 4),
              ("se_ard_n150_d20_p11-grad32_pm8_output_chunks", O.SE_ARD, 150, 20, 0, 11, 4),
              ("matern52_n700_d40_p1-grad64_spilled_pm1", O.MATERN52, 700, 40, 0, 1, 3),
              ("matern32_n333_d24_p2-grad32_pm8", O.MATERN32, 333, 24, 0, 2, 3),
              ("exp_n257_d62_p3-build64_grad64_pm8_top_of_range", O.EXP, 257, 62, 0, 3, 3),
              ("se_ard_lam1_n300_d16_p1-kpD17_lam32", O.SE_ARD, 300, 16, 1, 1, 3),
              ("se_ard_lam2_n600_d20_p2-lam32_and_grad32_pm8", O.SE_ARD, 600, 20, 2, 2, 3),
              ("se_ard_lam2_n200_d21_p1-65_gradient_entries", O.SE_ARD, 200, 21, 2, 1, 3)]

# batched sequences (test_gpu_high_dim.py::test_gpu_batch_high_dim): (id, kind, N, D, G)
BATCH_CASES = [("se_ard_n700_d20_g3-batched_build_wide32", O.SE_ARD, 700, 20, 3),
               ("matern52_n640_d40_g5-batched_generated_tiles", O.MATERN52, 640, 40, 5)]

GROWTH = (O.SE_ARD, 250, 270, 20, 2)  # kind, n0, n1, Din, k: add_sample across 256 samples and the capacity growth


def full_problem(kind, N, D, k, P, seed):
    return problem(kind, N, D, P=P, k=k, seed=seed, noise=0.02)


def batch_problem(kind, N, D, g):
    return problem(kind, N, D, P=1, seed=10 + g, noise=0.01)


def growth_problem():
    kind, n0, n1, D, k = GROWTH
    return problem(kind, n1, D, P=1, k=k, seed=6, noise=0.02)


def plan(n, p=1, g=1):
    """gpe_debug_tail_plan (host logic of engine.hip, no device): where K is built and how it is factorised."""
    import ctypes

    from limbo_amd import _capi

    f = ctypes.CDLL(str(_capi.ENGINE_SO)).gpe_debug_tail_plan
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                  ctypes.POINTER(ctypes.c_int64)]
    out = (ctypes.c_int64 * 8)()
    assert f(n, p, g, 0, 0, 0, out) == 0
    return dict(zip(("t0", "e0", "nt_tail", "nb_tail", "nt_tall", "nb_tall", "n64", "nbo"), list(out)))


def high_dim_goldens():
    """The mpmath goldens above 16 input dimensions (oracle/make_golden.py: hd_specs, mp_11 on)."""
    return [p for p in golden_files("mp_") if int(p.stem[3:5]) >= 11]


def check_golden_grad_per_component(lib, path):
    """Every gradient entry against the 50-digit one: TOL_GRAD relative, floor 1e-3 ||g_ref||_inf (an entry a thousand
    times below the largest is held to 1e-9 of the largest).  The C oracle passes with a margin above 5000x (<= 2e-13)."""
    g = load(path)
    h = new_gp(lib, g["kind"], g["X"], g["obs_mean"], g["theta"], g["noise"])
    assert h.compute() == 0
    grad, ref = h.log_lik_grad(bool(g["optimize_noise"])), g["grad"]
    h.close()
    assert grad.size == ref.size == g["theta"].size + int(bool(g["optimize_noise"]))
    err = grad_component_err(grad, ref)
    assert np.max(err) < PC.TOL_GRAD, (int(np.argmax(err)), float(np.max(err)))


def grad_component_err(g, ref):
    """Per-component relative error of a gradient, floor 1e-3 ||ref||_inf."""
    return np.abs(g - ref) / np.maximum(np.abs(ref), 1e-3 * np.max(np.abs(ref)))
