#!/usr/bin/env python
"""Timing of the two-objective expected hypervolume improvement (include/gpe_ehvi.h) — one JSON file, one entry per shape.

SE-ARD, D = 6, P = 2 (the objectives are the model's two outputs), var_add = the kernel's noise, partials asked for, for
(N, candidates, front) in {(16384, 16384, 1024), (4096, 4096, 128)}.  Per shape, in ONE process:

  ehvi        gpe_ehvi2_batch, host to host (time.perf_counter around the call; ehvi and partials read back), median of 5 after a
              warm-up, and its three phases (gpe_ehvi_phase_ms: the solves, the strip kernel, the read-back).  `strips_per_s` =
              M (n + 2) over the kernel phase.
  baseline    the route the library offered before: gpe_query_batch returning mu and var to the host (median of 5 after a warm-up) and
              the strip sum with its partials in numpy there (tests/ehvi_ref.py, in slices of 2048 candidates; median of 5).
              `same_values`: the largest relative difference between the two routes where the value is >= 1e-280.

    python profiles/ehvi_timing.py [--shape 0|1] [--out profiles/ehvi_timing.json]      (an existing file is extended)
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(16384, 16384, 1024), (4096, 4096, 128)]
REPS, D, NOISE, SLICE = 5, 6, 0.01, 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", type=int, default=None)
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    from limbo_amd import _capi
    from tests import ehvi_ref as R

    eng = _capi.load_engine()
    out = {"what": f"SE-ARD D = {D}, P = 2, var_add = noise, with partials; ms; host to host unless a phase", "shapes": {}}
    if a.out and Path(a.out).exists():
        out = json.loads(Path(a.out).read_text())
    for N, M, n in (SHAPES if a.shape is None else [SHAPES[a.shape]]):
        rng = np.random.default_rng(N + M + n)
        X, V = rng.random((N, D)), rng.random((M, D))
        Y = np.stack([np.sin(3.0 * X @ rng.random(D)), np.cos(3.0 * X @ rng.random(D))], axis=1) + 0.1 * rng.standard_normal((N, 2))
        om = Y - Y.mean(axis=0)
        # a front of n points on a quarter circle that reaches into the upper range of the (centred) observations
        x = np.sort(rng.uniform(0.02, 0.98, size=n))
        F = np.stack([x, np.sqrt(1.0 - x * x)], axis=1) * 1.2 - 0.4
        ref = (-0.5, -0.5)
        h = _capi.Handle(eng)
        h.set_data(X, om)
        h.set_kernel(_capi.KERNEL_SE_ARD, np.log([0.3, 0.45, 0.6, 0.75, 0.9, 1.0, 1.0]), NOISE)
        assert h.compute() == 0
        h.set_profiling(True)
        t, phases = [], []
        for r in range(1 + REPS):  # (r = 0: the warm-up)
            t0 = time.perf_counter()
            rc, e, p, _, _ = h.ehvi2_batch(V, F, ref, var_add=NOISE, want=("ehvi", "partials"))
            dt = time.perf_counter() - t0
            assert rc == 0
            if r:
                t.append(dt * 1e3)
                phases.append(h.ehvi_phase_ms())
        ph = {k: float(np.median([q[k] for q in phases])) for k in phases[0]}
        rec = {"ehvi_ms": float(np.median(t)), "phases_ms": ph, "strips_per_s": M * (n + 2.0) / (ph["kernel"] * 1e-3),
               "kernel_share_of_call": ph["kernel"] / float(np.median(t)), "ehvi_max": float(e.max()), "ehvi_median": float(np.median(e))}
        # the baseline: mu and var to the host, the strip sum there
        tq, ts = [], []
        for r in range(1 + REPS):
            t0 = time.perf_counter()
            kta, var = h.query_batch(V)
            t1 = time.perf_counter()
            sd = np.sqrt(np.where(var > np.finfo(float).eps, var, 0.0) + NOISE)
            val, part = np.zeros(M), np.zeros((M, 4))
            for m0 in range(0, M, SLICE):
                sl = slice(m0, min(M, m0 + SLICE))
                val[sl], part[sl] = R.ref_ehvi(F, ref, kta[sl, 0], sd[sl], kta[sl, 1], sd[sl])
            t2 = time.perf_counter()
            if r:
                tq.append((t1 - t0) * 1e3)
                ts.append((t2 - t1) * 1e3)
        big = val >= 1e-280
        rec["baseline"] = {"query_batch_ms": float(np.median(tq)), "numpy_strip_sum_ms": float(np.median(ts)),
                           "total_ms": float(np.median(tq)) + float(np.median(ts)),
                           "same_values": float(np.max(np.abs(e[big] - val[big]) / val[big])) if big.any() else 0.0}
        rec["speedup_over_baseline"] = rec["baseline"]["total_ms"] / rec["ehvi_ms"]
        out["shapes"][f"{N}x{M}x{n}"] = rec
        h.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
