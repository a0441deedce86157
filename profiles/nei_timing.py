#!/usr/bin/env python
"""Timing of noisy expected improvement in the log domain (include/gpe_nei.h) — one JSON file, one entry per shape.

SE-ARD, D = 6, one output, kernel noise 0.01, jitter 1e-6, xi 0.01, for (N, B, S, candidates) in {(16384, 256, 256, 16384),
(4096, 128, 64, 4096)}.  The baseline: the B best observed points.  Per shape, in ONE process:

  fused        gpe_lognei_batch, host to host (time.perf_counter around the call; lognei read back), and its five phases
               (gpe_nei_phase_ms: the baseline's pass and Sigma_b; its factorisation and the draws; the candidates' solves with the
               cross-covariance; the conditioning; the kernel and the read-back); medians of 5 after three warm-ups
  query        gpe_query_batch alone on the same candidates, mu and var to the host, timed behind the fused call; median of 5
  kg+numpy     what the library offered before for the same answer: gpe_kg_batch returning the cross-covariance (B x M) and var to the
               host and gpe_joint_query the baseline's mean and covariance (medians of 5), then on the host Sigma_b's factor, the draws,
               u = L_b^-1 c, cmean, cvar (numpy / LAPACK) and tests/nei_ref.py's ref_lognei: ONE run (its continued fraction runs to
               depth 400 over S M elements)
               `same_values`: the largest |fused - numpy| / max(1, |numpy|) over lognei — the device's worst error in this run, end to end

    python profiles/nei_timing.py [--shape 0|1] [--out profiles/nei_timing.json]      (an existing file is extended)
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(16384, 256, 256, 16384), (4096, 128, 64, 4096)]
REPS, WARM, D, NOISE, JITTER, XI = 5, 3, 6, 0.01, 1e-6, 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", type=int, default=None)
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import scipy.linalg as sla

    from limbo_amd import _capi
    from tests import nei_ref as R

    eng = _capi.load_engine()
    out = {"what": f"SE-ARD D = {D}, one output, noise {NOISE}, jitter {JITTER}; ms; host to host unless a phase; medians of 5 after three "
                   "warm-ups, the numpy epilogue one run", "shapes": {}}
    if a.out and Path(a.out).exists():
        out = json.loads(Path(a.out).read_text())
    for N, B, S, M in (SHAPES if a.shape is None else [SHAPES[a.shape]]):
        rng = np.random.default_rng(N + B + S + M)
        X, V = rng.random((N, D)), rng.random((M, D))
        Y = 0.3 * np.sin(3.0 * X @ rng.random(D)) + 0.1 * rng.standard_normal(N)
        om = (Y - Y.mean())[:, None]
        Xb = X[np.argsort(-om[:, 0], kind="stable")[:B]]
        Z = np.asfortranarray(rng.standard_normal((B, S)))
        h = _capi.Handle(eng)
        h.set_data(X, om)
        h.set_kernel(_capi.KERNEL_SE_ARD, np.log([0.5] * D + [1.0]), NOISE)
        assert h.compute() == 0
        h.set_profiling(True)

        def timed(fn, warm=WARM):
            ts, res = [], None
            for r in range(warm + REPS):  # (r < warm: the warm-ups)
                t0 = time.perf_counter()
                res = fn()
                if r >= warm:
                    ts.append((time.perf_counter() - t0) * 1e3)
            return float(np.median(ts)), res

        t, phases, ln = [], [], None
        for r in range(WARM + REPS):
            t0 = time.perf_counter()
            rc, ln, *_ = h.lognei_batch(V, Xb, Z, 0, JITTER, XI, want=("lognei",))
            dt = time.perf_counter() - t0
            assert rc == 0
            if r >= WARM:
                t.append(dt * 1e3)
                phases.append(h.nei_phase_ms())
        ph = {k: float(np.median([q[k] for q in phases])) for k in phases[0]}
        fused = float(np.median(t))
        rec = {"fused_ms": fused, "phases_ms": ph, "kernel_share_of_call": ph["kernel"] / fused, "terms_per_s_in_kernel_phase": M * S / (ph["kernel"] * 1e-3),
               "lognei_max": float(ln.max()), "lognei_median": float(np.median(ln)), "lognei_min": float(ln.min()),
               "plain_value_is_zero": float(np.mean(np.exp(ln) == 0.0))}
        tq, (kta, var) = timed(lambda: h.query_batch(V))  # (behind the fused call: the first calls after compute() are slower)
        tk, (_, _, var_c, cov) = timed(lambda: h.kg_batch(Xb, V, NOISE, want=("var", "cov")))
        tj, (kb, Sig) = timed(lambda: h.joint_query(Xb, JITTER))
        t1 = time.perf_counter()
        Lb = sla.cholesky(Sig, lower=True)
        fplus = (kb[:, 0][:, None] + Lb @ Z).max(axis=0)
        U = sla.solve_triangular(Lb, cov, lower=True)
        cmean = kta[:, 0][None, :] + Z.T @ U
        cvar = var_c - np.sum(U * U, axis=0)
        sd = np.sqrt(np.where(cvar > np.finfo(float).eps, cvar, 0.0))
        t2 = time.perf_counter()
        val, _ = R.ref_lognei(fplus, XI, cmean, sd)
        t3 = time.perf_counter()
        same = float(R.err(ln, val).max())
        rec["query_batch_ms"] = tq
        rec["kg_plus_numpy"] = {"kg_batch_cov_to_host_ms": tk, "joint_query_baseline_ms": tj, "numpy_conditioning_ms": (t2 - t1) * 1e3,
                                "numpy_log_ei_ms": (t3 - t2) * 1e3, "total_ms": tk + tj + (t3 - t1) * 1e3, "same_values": same}
        rec["fused_over_query_batch"] = fused / tq
        rec["speedup_over_kg_plus_numpy"] = rec["kg_plus_numpy"]["total_ms"] / fused
        out["shapes"][f"{N}xB{B}xS{S}x{M}"] = rec
        h.close()
        if a.out:
            Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
