#!/usr/bin/env python
"""Timing of max-value entropy search in the log domain (include/gpe_mes.h) — one JSON file, one entry per shape.

SE-ARD, D = 6, P = J outputs, var_add = the kernel's noise, terms and partials asked for, for (N, candidates, K, J) in
{(16384, 16384, 64, 1), (4096, 4096, 64, 1), (4096, 4096, 1024, 3)}.  The K sampled maxima of an output lie up to 1.5 median standard
deviations above its best posterior mean over the candidates.  Per shape, in ONE process:

  fused        gpe_mes_batch, host to host (time.perf_counter around the call; logmes, terms and partials read back), and its three
               phases (gpe_mes_phase_ms: the solves, the kernel, the read-back); medians of 5 after a warm-up
  query        gpe_query_batch alone, returning mu (M x J) and var to the host: what the fused call adds the kernel to; median of 5
  query+numpy  that gpe_query_batch, then tests/mes_ref.py's ref_mes on the host: ONE run (its continued fraction runs to depth 400
               over M J K elements: seconds to a minute)
               `same_values`: the largest |fused - numpy| / max(1, |numpy|) over values, terms and partials

    python profiles/mes_timing.py [--shape 0|1|2] [--out profiles/mes_timing.json]      (an existing file is extended)
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(16384, 16384, 64, 1), (4096, 4096, 64, 1), (4096, 4096, 1024, 3)]
REPS, D, NOISE = 5, 6, 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", type=int, default=None)
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    from limbo_amd import _capi
    from tests import mes_ref as R

    eng = _capi.load_engine()
    out = {"what": f"SE-ARD D = {D}, P = J outputs, var_add = noise, with terms and partials; ms; host to host unless a phase; medians of 5 "
                   "after a warm-up, the numpy epilogue one run", "shapes": {}}
    if a.out and Path(a.out).exists():
        out = json.loads(Path(a.out).read_text())
    for N, M, K, J in (SHAPES if a.shape is None else [SHAPES[a.shape]]):
        rng = np.random.default_rng(N + M + K + J)
        X, V = rng.random((N, D)), rng.random((M, D))
        Y = np.stack([np.sin(3.0 * X @ rng.random(D) + j) for j in range(J)], axis=1) + 0.1 * rng.standard_normal((N, J))
        om = Y - Y.mean(axis=0)
        h = _capi.Handle(eng)
        h.set_data(X, om)
        h.set_kernel(_capi.KERNEL_SE_ARD, np.log([0.3, 0.45, 0.6, 0.75, 0.9, 1.0, 1.0]), NOISE)
        assert h.compute() == 0
        h.set_profiling(True)
        tq = []
        for r in range(1 + REPS):  # (r = 0: the warm-up)
            t0 = time.perf_counter()
            kta, var = h.query_batch(V)
            if r:
                tq.append((time.perf_counter() - t0) * 1e3)
        sd = np.sqrt(np.where(var > np.finfo(float).eps, var, 0.0) + NOISE)
        ystar = kta.max(axis=0)[None, :] + np.median(sd) * rng.uniform(0.0, 1.5, (K, J))
        t, phases = [], []
        for r in range(1 + REPS):
            t0 = time.perf_counter()
            rc, lm, tm, p, _, _ = h.mes_batch(V, ystar, None, None, NOISE, want=("logmes", "terms", "partials"))
            dt = time.perf_counter() - t0
            assert rc == 0
            if r:
                t.append(dt * 1e3)
                phases.append(h.mes_phase_ms())
        ph = {k: float(np.median([q[k] for q in phases])) for k in phases[0]}
        rec = {"fused_ms": float(np.median(t)), "phases_ms": ph, "kernel_share_of_call": ph["kernel"] / float(np.median(t)),
               "candidates_per_s_in_kernel": M / (ph["kernel"] * 1e-3), "terms_per_s_in_kernel": M * J * K / (ph["kernel"] * 1e-3),
               "logmes_max": float(lm.max()), "logmes_median": float(np.median(lm)), "logmes_min": float(lm.min())}
        t1 = time.perf_counter()
        val, terms, part = R.ref_mes(ystar, kta, np.tile(sd[:, None], (1, J)))
        ts = (time.perf_counter() - t1) * 1e3
        same = max(float(R.err(g, w).max()) for g, w in ((lm, val), (tm, terms), (p, part)))
        rec["query_batch_ms"] = float(np.median(tq))
        rec["query_plus_numpy"] = {"numpy_epilogue_ms": ts, "total_ms": float(np.median(tq)) + ts, "same_values": same}
        rec["fused_over_query_batch"] = rec["fused_ms"] / rec["query_batch_ms"]
        rec["speedup_over_query_plus_numpy"] = rec["query_plus_numpy"]["total_ms"] / rec["fused_ms"]
        out["shapes"][f"{N}x{M}xK{K}xJ{J}"] = rec
        h.close()
        if a.out:
            Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
