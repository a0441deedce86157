#!/usr/bin/env python
"""Timing of the batched posterior with its gradient in the query point (include/gpe_query_grad.h) — one JSON line.

For N in {1024, 4096, 16384} and M in {64, 4096}, SE-ARD, D = 6, P = 1: gpe_query_batch_grad (all four outputs) against
gpe_query_batch (both outputs) on the same handle in the same process, the two alternating call by call — host clock around
calls that end in a stream wait, median of 10 pairs after 2 warm-up pairs, profiling off.  Then, with gpe_set_profiling on, the
three phases of the gradient call (gpe_query_grad_phase_ms: forward part, backward solve, gradient kernel with its fold), median
of 5 calls.  `ratio` = grad / query; `cd_queries` = 2 D + 1, the queries a central-difference gradient of the same batch costs;
`vs_cd` = grad / (cd_queries x query).  Where ratio > 3, `responsible` names the phase that is largest.

    python tools/query_grad_timing.py [--out profiles/query_grad_timing.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NS, MS, D = (1024, 4096, 16384), (64, 4096), 6
REPS, WARM, PREPS = 10, 2, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np

    sys.path.insert(0, str(ROOT))
    from limbo_amd import _capi

    eng = _capi.load_engine()
    shapes = {}
    for N in NS:
        rng = np.random.default_rng(N)
        X = rng.random((N, D))
        y = np.sin(3.0 * X @ rng.random(D)) + 0.1 * rng.standard_normal(N)
        h = _capi.Handle(eng)
        h.set_data(X, y - y.mean())
        h.set_kernel(_capi.KERNEL_SE_ARD, np.log([0.3, 0.45, 0.6, 0.75, 0.9, 1.0, 1.0]), 0.01)
        assert h.compute() == 0
        for M in MS:
            V = rng.random((M, D))
            tq, tg = [], []
            for r in range(WARM + REPS):
                t0 = time.perf_counter()
                h.query_batch(V)
                t1 = time.perf_counter()
                h.query_batch_grad(V)
                t2 = time.perf_counter()
                if r >= WARM:
                    tq.append((t1 - t0) * 1e3)
                    tg.append((t2 - t1) * 1e3)
            h.set_profiling(True)
            rows = []
            for r in range(1 + PREPS):
                h.query_batch_grad(V)
                if r >= 1:
                    rows.append(h.query_grad_phase_ms())
            h.set_profiling(False)
            ph = {k: float(np.median([q[k] for q in rows])) for k in rows[0]}
            q_ms, g_ms = float(np.median(tq)), float(np.median(tg))
            row = {"query_ms": q_ms, "grad_ms": g_ms, "ratio": g_ms / q_ms, "query_spread": float((max(tq) - min(tq)) / q_ms),
                   "grad_spread": float((max(tg) - min(tg)) / g_ms), "phase_ms": ph, "cd_queries": 2 * D + 1,
                   "vs_cd": g_ms / ((2 * D + 1) * q_ms),
                   "solve_tflops": {"forward": float(M) * N * N / (ph["forward"] * 1e-3) / 1e12 if ph["forward"] > 0 else None,
                                    "backward": float(M) * N * N / (ph["backward"] * 1e-3) / 1e12 if ph["backward"] > 0 else None}}
            if row["ratio"] > 3.0:
                row["responsible"] = max(ph, key=ph.get)
            shapes[f"{N}x{M}"] = row
        assert h.flow_retries() == 0 and h.handover_reruns() == 0
        h.close()
    res = {"what": "gpe_query_batch_grad (four outputs) against gpe_query_batch, SE-ARD D = 6 P = 1, same process, alternating; host "
                   "clock, median of 10 after 2 warm-ups; phases with profiling on, median of 5", "shapes": shapes}
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
