#!/usr/bin/env python
"""Timing of the three-objective expected hypervolume improvement (include/gpe_ehvi3.h) — one JSON file, one entry per shape.

SE-ARD, D = 6, P = 3 (the objectives are the model's three outputs), var_add = the kernel's noise, value and partials read back, for
(N, candidates, front) in {(16384, 16384, 1024), (4096, 4096, 128)}.  Per shape, in ONE process:

  ehvi3       gpe_ehvi3_batch, host to host (time.perf_counter around the call, which builds the three box tables on the host and
              reads ehvi and partials back), median of 5 after a warm-up, and its three phases (gpe_ehvi3_phase_ms: the solves, the
              box kernel, the read-back).  `boxes_per_s` = M x (the boxes of the three tables) over the kernel phase;
              `tables_host_ms`: gpe_ehvi3_boxes for the three axes alone, median of 5.
  baseline    the route the library offered before: gpe_query_batch returning mu and var to the host (median of 5 after a warm-up) and
              the three box sums with their partials in numpy there (tests/ehvi3_ref.py, in slices of 1024 candidates; median of
              --numpy-reps runs, recorded: one run of the large shape is tens of seconds of host arithmetic).
              `same_values`: the largest relative difference between the two routes where the value is >= 1e-280.

    python profiles/ehvi3_timing.py [--shape 0|1] [--numpy-reps K] [--out profiles/ehvi3_timing.json]      (an existing file is extended)
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(16384, 16384, 1024), (4096, 4096, 128)]
REPS, D, NOISE, SLICE = 5, 6, 0.01, 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", type=int, default=None)
    ap.add_argument("--numpy-reps", type=int, default=REPS)
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    from limbo_amd import _capi
    from tests import ehvi3_ref as R

    eng = _capi.load_engine()
    out = {"what": f"SE-ARD D = {D}, P = 3, var_add = noise, with partials; ms; host to host unless a phase", "shapes": {}}
    if a.out and Path(a.out).exists():
        out = json.loads(Path(a.out).read_text())
    for N, M, n in (SHAPES if a.shape is None else [SHAPES[a.shape]]):
        rng = np.random.default_rng(N + M + n)
        X, V = rng.random((N, D)), rng.random((M, D))
        Y = np.stack([np.sin(3.0 * X @ rng.random(D)), np.cos(3.0 * X @ rng.random(D)), np.sin(2.0 * X @ rng.random(D) + 1.0)], axis=1)
        Y = Y + 0.1 * rng.standard_normal((N, 3))
        om = Y - Y.mean(axis=0)
        # a front of n points on the unit sphere's positive octant, scaled to reach into the upper range of the (centred) observations
        P = np.abs(rng.standard_normal((n, 3)))
        P = P / np.linalg.norm(P, axis=1, keepdims=True)
        ref = (-0.5, -0.5, -0.5)
        rc, F = _capi.ehvi3_front(P * 1.3 - 0.4, ref)
        assert rc == 0 and len(F) == n
        t = []
        for r in range(1 + REPS):
            t0 = time.perf_counter()
            boxes = [len(_capi.ehvi3_boxes(F, ref, c)[1]) for c in range(3)]
            if r:
                t.append((time.perf_counter() - t0) * 1e3)
        tables_ms = float(np.median(t))
        h = _capi.Handle(eng)
        h.set_data(X, om)
        h.set_kernel(_capi.KERNEL_SE_ARD, np.log([0.3, 0.45, 0.6, 0.75, 0.9, 1.0, 1.0]), NOISE)
        assert h.compute() == 0
        h.set_profiling(True)
        t, phases = [], []
        for r in range(1 + REPS):  # (r = 0: the warm-up)
            t0 = time.perf_counter()
            rc, e, p, _, _ = h.ehvi3_batch(V, F, ref, var_add=NOISE, want=("ehvi", "partials"))
            dt = time.perf_counter() - t0
            assert rc == 0
            if r:
                t.append(dt * 1e3)
                phases.append(h.ehvi3_phase_ms())
        ph = {k: float(np.median([q[k] for q in phases])) for k in phases[0]}
        rec = {"ehvi3_ms": float(np.median(t)), "phases_ms": ph, "boxes": boxes, "tables_host_ms": tables_ms,
               "boxes_per_s": M * float(sum(boxes)) / (ph["kernel"] * 1e-3), "kernel_share_of_call": ph["kernel"] / float(np.median(t)),
               "ehvi_max": float(e.max()), "ehvi_median": float(np.median(e))}
        # the baseline: mu and var to the host, the box sums there
        tq, ts = [], []
        for r in range(1 + REPS):
            t0 = time.perf_counter()
            kta, var = h.query_batch(V)
            if r:
                tq.append((time.perf_counter() - t0) * 1e3)
        sd = np.sqrt(np.where(var > np.finfo(float).eps, var, 0.0) + NOISE)
        for r in range(a.numpy_reps):
            t0 = time.perf_counter()
            val, part = np.zeros(M), np.zeros((M, 6))
            for m0 in range(0, M, SLICE):
                sl = slice(m0, min(M, m0 + SLICE))
                val[sl], part[sl] = R.ref_ehvi3(F, ref, kta[sl], np.stack([sd[sl]] * 3, axis=1))
            ts.append((time.perf_counter() - t0) * 1e3)
        big = val >= 1e-280
        rec["baseline"] = {"query_batch_ms": float(np.median(tq)), "numpy_box_sums_ms": float(np.median(ts)), "numpy_reps": a.numpy_reps,
                           "total_ms": float(np.median(tq)) + float(np.median(ts)),
                           "same_values": float(np.max(np.abs(e[big] - val[big]) / val[big])) if big.any() else 0.0,
                           "same_partials": float(np.max(np.abs(p - part) / np.maximum(part, 1e-280)))}
        rec["speedup_over_baseline"] = rec["baseline"]["total_ms"] / rec["ehvi3_ms"]
        out["shapes"][f"{N}x{M}x{n}"] = rec
        h.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
