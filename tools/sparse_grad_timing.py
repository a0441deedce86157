#!/usr/bin/env python
"""Timing of the sparse pseudo-input GP's analytic gradient (include/gpe_sparse_grad.h) — one JSON line.

For N = 131 072, D = 6, M in {512, 1024, 2048} (and N = 1 048 576, M = 1024 with --full), host to host, median of REPS calls after
one warm-up:
  (a) gpe_sp_objective                      the model and its likelihood: what ONE evaluation of the fit by central differences cost
  (b) gpe_sp_objective_grad with d_xb       the model, its likelihood and all (M + 1) D + 2 derivatives
  (c) the gradient's phases (gpe_sp_grad_phase_ms under profiling, a separate run)
The comparison that matters is (b) against (2 (D + 2) + 1) x (a): one optimiser step of the fit by central differences in the
D + 2 log-parameters alone.  gpe_sp_objective is the same code before and after the gradient was added, so (a) measured here is
what the parent commit pays.  The products phase is the model's solve for V (N M^2 flop) and three full products (2 N M^2 each):
7 N M^2 flop (of_peak: against the engine's own gpe_mfma_f64_peak; the phase holds the two cross kernels as well); k_sp_gcol reads
two of the chunk's buffers and k_sp_grow three, 5 x 8 N M bytes (of_stream: against the engine's own gpe_hbm_stream_peak).

    python tools/sparse_grad_timing.py [--out profiles/sparse_grad_timing.json] [--full]
"""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from limbo_amd import _capi  # noqa: E402

MS, D, REPS = [512, 1024, 2048], 6, 5
ELL = np.array([0.3, 0.45, 0.6, 0.75, 0.9, 1.0])


def median_ms(fn):
    ts = []
    for _ in range(1 + REPS):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[1:])), float((max(ts[1:]) - min(ts[1:])) / np.median(ts[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--full", action="store_true", help="N = 1 048 576, M = 1024 as well")
    a = ap.parse_args()
    eng = _capi.load_engine()
    peak, stream = ctypes.c_double(), ctypes.c_double()
    assert eng.fn("mfma_f64_peak")(0, ctypes.byref(peak)) == 0
    assert eng.fn("hbm_stream_peak")(0, ctypes.byref(stream)) == 0
    res = {"what": f"gpe_sp_objective (a), gpe_sp_objective_grad with d_xb (b), the gradient's phases (c); SE-ARD D = {D}, c = 1, sig = 0.01, "
                   f"jitter 1e-6; host to host, median of {REPS} after 1 warm-up; ms",
           "peak_tflops": peak.value, "hbm_stream_gbs": stream.value, "shapes": {}}
    hp = (-2.0 * np.log(ELL), 0.0, float(np.log(0.01)), 1e-6)
    for N, M in [(131072, m) for m in MS] + ([(1048576, 1024)] if a.full else []):
        rng = np.random.default_rng(N + M)
        X = rng.random((N, D))
        y = np.sin(3.0 * X @ rng.random(D)) + 0.1 * rng.standard_normal(N)
        h = _capi.SparseHandle(eng)
        h.set_data(X, y - y.mean())
        h.set_pseudo(X[rng.permutation(N)[:M]] + 0.01 * rng.standard_normal((M, D)))

        def obj():
            assert h.objective(*hp)[0] == 0

        def obj_grad():
            assert h.objective_grad(None, *hp)[0] == 0

        t_a, s_a = median_ms(obj)
        t_b, s_b = median_ms(obj_grad)
        h.set_profiling(True)
        rows = []
        for r in range(1 + REPS):
            assert h.grad()[0] == 0
            if r:
                rows.append(h.grad_phase_ms())
        h.close()
        ph = {k: float(np.median([q[k] for q in rows])) for k in rows[0]}
        evals = 2 * (D + 2) + 1
        res["shapes"][f"{N}x{M}"] = {
            "objective_ms": t_a, "objective_spread": s_a, "objective_grad_ms": t_b, "objective_grad_spread": s_b,
            "grad_over_objective": t_b / t_a, "central_difference_step_ms": evals * t_a, "step_speedup": evals * t_a / t_b,
            "phases_ms": ph,
            "products_of_peak": 7.0 * N * M * M / (ph["products"] * 1e-3) / (peak.value * 1e12),
            "rows_of_stream": 5 * 8.0 * N * M / (ph["rows"] * 1e-3) / (stream.value * 1e9),
            "tt_of_peak": 1.0 * N * M * M / (ph["tt"] * 1e-3) / (peak.value * 1e12)}
        print(f"{N}x{M}: objective {t_a:.2f} ms, objective_grad {t_b:.2f} ms ({t_b / t_a:.2f} x; {evals} evaluations: {evals * t_a:.1f} ms), phases {ph}",
              file=sys.stderr)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
