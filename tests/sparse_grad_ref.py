"""References of the sparse pseudo-input GP's gradient (include/gpe_sparse_grad.h) — the checker of tests/test_sparse_grad_host.py
and tests/test_gpu_sparse_grad.py.  Never the engine.  Two independent routes to the gradient of F = sum_p nlml_p with respect
to the pseudo-inputs' raw coordinates, log b, log c and log sig:

  ref_grad       the reference's own sequence, src/limbo/experimental/model/spgp.hpp:453-580, in numpy (P = 1, O(N M^2));
  autograd_grad  torch autograd on the CPU in float64 through the dense FITC definition of tests/sparse_ref.route_b, F summed
                 over the outputs, any P (an N x N Cholesky: N <= 1500).

Both return (F, d_xb (M x D), d_log_b (D), d_log_c, d_log_sig).  `python -m tests.sparse_grad_ref` prints their disagreement."""
import numpy as np
import scipy.linalg as sla

from tests import sparse_ref as R

P1_SHAPES = [(700, 40, 3, 1), (1500, 320, 6, 1), (900, 256, 20, 1)]


def ref_grad(X, Xb, y, log_b, log_c, log_sig, jitter):
    assert y.shape[1] == 1
    n, D = X.shape
    m = Xb.shape[0]
    b, c, sig = np.exp(np.asarray(log_b)), np.exp(log_c), np.exp(log_sig)
    xb, x = Xb * np.sqrt(b), X * np.sqrt(b)                                                  # :459-462
    Q = R.kern(Xb, Xb, log_b, log_c) + jitter * np.eye(m)                                    # :467
    K = R.kern(Xb, X, log_b, log_c)                                                          # :470
    L = np.linalg.cholesky(Q)
    V = sla.solve_triangular(L, K, lower=True)                                               # :474
    ep = 1.0 + (c - (V * V).sum(0)) / sig                                                    # :475
    rs = 1.0 / np.sqrt(ep)
    K, V, yy = K * rs, V * rs, y[:, 0] * rs                                                  # :477-479
    Lm = np.linalg.cholesky(sig * np.eye(m) + V @ V.T)                                       # :482
    invLmV = sla.solve_triangular(Lm, V, lower=True)
    bet = invLmV @ yy                                                                        # :484
    fw = (np.log(np.diag(Lm)).sum() + 0.5 * (n - m) * log_sig + (yy @ yy - bet @ bet) / (2 * sig) + np.log(ep).sum() / 2
          + 0.5 * n * np.log(2 * np.pi))                                                     # :491, the real (n - m) / 2
    Lt = L @ Lm                                                                              # :501
    B1 = sla.solve_triangular(Lt.T, invLmV, lower=False)                                     # :502
    b1 = sla.solve_triangular(Lt.T, bet, lower=False)                                        # :503
    invLV = sla.solve_triangular(L.T, V, lower=False)                                        # :504
    invL = np.linalg.inv(L)
    invQ = invL.T @ invL
    invLt = np.linalg.inv(Lt)
    invA = invLt.T @ invLt                                                                   # :505-507
    mu = sla.solve_triangular(Lm.T, bet, lower=False) @ V                                    # :509
    sumVsq = (V * V).sum(0)
    bigsum = yy * (bet @ invLmV) / sig - (invLmV * invLmV).sum(0) / 2 - (yy * yy + mu * mu) / (2 * sig) + 0.5  # :515-517
    TT = invLV @ (invLV.T * bigsum[:, None])                                                 # :518
    dfxb, dfb = np.zeros((m, D)), np.zeros(D)
    for i in range(D):                                                                       # :522-553
        dnnQ = (xb[:, i][:, None] - xb[:, i][None, :]) * Q
        dNnK = (x[:, i][None, :] - xb[:, i][:, None]) * K
        epdot = dNnK * invLV * (-2.0 / sig)
        epPmod = -epdot.sum(0)
        dfxb[:, i] = (-b1 * (dNnK @ (yy - mu) / sig + dnnQ @ b1) + ((invQ - invA * sig) * dnnQ).sum(1) + epdot @ bigsum
                      - 2.0 / sig * (dnnQ * TT).sum(1))
        dfb[i] = ((yy - mu) * (b1 @ dNnK) / sig + epPmod * bigsum) @ x[:, i]
        dNnK = dNnK * B1
        dfxb[:, i] += dNnK.sum(1)
        dfb[i] -= dNnK.sum(0) @ x[:, i]
        dfxb[:, i] *= np.sqrt(b[i])
        dfb[i] /= np.sqrt(b[i])
        dfb[i] += dfxb[:, i] @ xb[:, i] / b[i]
        dfb[i] *= np.sqrt(b[i]) / 2
    epc = (c / ep - sumVsq - jitter * (invLV * invLV).sum(0)) / sig                          # :554-556
    dfc = ((m + jitter * np.trace(invQ - sig * invA) - sig * (invA * Q.T).sum()) / 2 - mu @ (yy - mu) / sig
           + b1 @ (Q - jitter * np.eye(m)) @ b1 / 2 + epc @ bigsum)                           # :557-560
    dfsig = (bigsum / ep).sum()                                                              # :562
    return float(fw), dfxb, dfb, float(dfc), float(dfsig)


def autograd_grad(X, Xb, y, log_b, log_c, log_sig, jitter):
    import torch

    t = lambda v: torch.tensor(np.asarray(v, dtype=np.float64), dtype=torch.float64)
    Xt, yt = t(X), t(y)
    xb, lb, lc, ls = (t(v).requires_grad_() for v in (Xb, log_b, log_c, log_sig))

    def kern(A, B):
        sb = torch.exp(0.5 * lb)
        a, bb = A * sb, B * sb
        d2 = (a * a).sum(1)[:, None] + (bb * bb).sum(1)[None, :] - 2.0 * a @ bb.T
        return torch.exp(lc) * torch.exp(-0.5 * d2)

    n, m, P = X.shape[0], Xb.shape[0], y.shape[1]
    eye = lambda k: torch.eye(k, dtype=torch.float64)
    Kmn = kern(xb, Xt)
    Qn = Kmn.T @ torch.linalg.solve(kern(xb, xb) + jitter * eye(m), Kmn)
    Sig = Qn + torch.diag(torch.exp(lc) - torch.diagonal(Qn)) + torch.exp(ls) * eye(n)
    Lc = torch.linalg.cholesky(0.5 * (Sig + Sig.T))
    F = P * torch.log(torch.diagonal(Lc)).sum() + 0.5 * (yt * torch.cholesky_solve(yt, Lc)).sum() + 0.5 * P * n * np.log(2 * np.pi)
    F.backward()
    return F.item(), xb.grad.numpy(), lb.grad.numpy(), lc.grad.item(), ls.grad.item()


def blocks(g):
    """(F, d_xb, d_log_b, d_log_c, d_log_sig) -> the three blocks the bars are stated on"""
    return dict(d_xb=np.asarray(g[1]), d_log_b=np.asarray(g[2]), d_c_sig=np.array([g[3], g[4]]))


def block_errors(got, ref):
    """max |a - b| / max |b| per block"""
    a, b = blocks(got), blocks(ref)
    return {k: float(np.max(np.abs(a[k] - b[k])) / np.max(np.abs(b[k]))) for k in b}


def off_the_data(pr, seed=3):
    """the pseudo-inputs moved off the data points (the subset itself is a special point)"""
    return pr["Xb"] + 0.02 * np.random.default_rng(seed).standard_normal(pr["Xb"].shape)


if __name__ == "__main__":
    for shape in P1_SHAPES:
        for jit in (1e-6, 1e-4):
            pr = R.make_problem(*shape, seed=7)
            args = (pr["X"], off_the_data(pr), pr["y"], pr["log_b"], pr["log_c"], pr["log_sig"], jit)
            print(shape, jit, {k: f"{v:.1e}" for k, v in block_errors(ref_grad(*args), autograd_grad(*args)).items()})
