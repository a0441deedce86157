"""tests/loo_ref.py (numpy / LAPACK, the checker of tests/test_gpu_loo_cv.py) without a GPU: against the C oracle at the six
shapes of tests/test_gpu_parity.py::test_gpu_loo_cv_vs_oracle, and its literal gradient against sum W o dK_j at N >= 1024.

Both are held to a HUNDREDTH of the bars the GPU tests hold the engine to (value 1e-9 relative, gradient 1e-6 in norm and per
component, weights and K^-1 1e-8 in norm), so that the checker's own error takes at most a hundredth of a bar.

Worst values seen (this file's output, -s):
  against the C oracle, 12 cases      value 3.6e-14 (bar 1e-11)   gradient 3.0e-13 in norm, 9.5e-13 per component (1e-8)
                                      weights 8.9e-13 (1e-10)     K^-1 4.3e-13 (1e-10)      (the worst: N = 333, exponential kernel)
  literal gradient against sum W o dK, N = 1100 (SE-ARD, D 3, P 3, noise entry included): 1.4e-15 in norm, 2.5e-14 per component (1e-8)
"""
import numpy as np
import pytest

from oracle import np_oracle as O
from tests import loo_ref as R
from tests.high_dim import grad_component_err
from tests.util import new_gp, relerr_norm

BAR_VALUE, BAR_GRAD, BAR_W, BAR_KINV = 1e-9 / 100, 1e-6 / 100, 1e-8 / 100, 1e-8 / 100
# N, D, P, kind of test_gpu_loo_cv_vs_oracle; both optimize_noise settings of each
SHAPES = [(40, 4, 2, O.SE_ARD), (130, 3, 1, O.MATERN52), (257, 6, 3, O.SE_ARD), (333, 2, 1, O.EXP), (200, 5, 8, O.MATERN32),
          (150, 3, 11, O.SE_ARD)]


@pytest.mark.parametrize("on", [False, True], ids=["noise_off", "noise_on"])
@pytest.mark.parametrize("N,D,P,kind", SHAPES, ids=["n%d_d%d_p%d_k%d" % s for s in SHAPES])
def test_reference_vs_c_oracle(oracle_lib, N, D, P, kind, on):
    X, Y, (th,) = R.make_problem(N, D, P, kind)
    om, _ = O.obs_mean_data(Y)
    ref = R.reference(kind, X, om, th, R.NOISE, on, want_W=True)
    o = new_gp(oracle_lib, kind, X, om, th, R.NOISE)
    assert o.compute() == 0
    lo, go, Wo, Ko = o.log_loo_cv(), o.log_loo_cv_grad(on), o.get_loo_weights(), o.get_Kinv()
    o.close()
    e_val = abs(ref.value - lo) / max(1.0, abs(lo))
    e_g, e_gc = relerr_norm(ref.grad, go), float(np.max(grad_component_err(ref.grad, go)))
    e_w, e_k = relerr_norm(ref.W, Wo), relerr_norm(ref.Kinv, Ko)
    print(f"N={N} D={D} P={P} kind={kind} noise={'on' if on else 'off'}: value {e_val:.2e}  grad {e_g:.2e} / component {e_gc:.2e}  "
          f"W {e_w:.2e}  Kinv {e_k:.2e}")
    assert ref.grad.size == go.size == th.size + on
    assert e_val <= BAR_VALUE
    assert e_g < BAR_GRAD and e_gc < BAR_GRAD
    assert e_w < BAR_W
    assert e_k < BAR_KINV


def test_literal_gradient_vs_weight_form_n1100():
    """The two functions of tests/loo_ref.py against each other above 1024 samples, noise entry included: the per-parameter
    Zeta products (loo_grad) and sum_ab W[a, b] dK_j[a, b] (loo_weights)."""
    N, D, P, kind = 1100, 3, 3, O.SE_ARD
    X, Y, (th,) = R.make_problem(N, D, P, kind)
    om, _ = O.obs_mean_data(Y)
    ref = R.reference(kind, X, om, th, R.NOISE, True, want_W=True)
    gw = np.array([np.sum(ref.W * dK) for dK in R.dK_list(kind, X, th, R.NOISE, True)])
    e_g, e_gc = relerr_norm(ref.grad, gw), float(np.max(grad_component_err(ref.grad, gw)))
    print(f"N={N}: literal gradient against sum W o dK: {e_g:.2e} in norm, {e_gc:.2e} per component; W asymmetry "
          f"{np.max(np.abs(ref.W - ref.W.T)):.1e}")
    assert ref.grad.size == D + 2
    assert e_g < BAR_GRAD and e_gc < BAR_GRAD
