#!/usr/bin/env python
"""Timing of constrained expected improvement in the log domain (include/gpe_cei.h) — one JSON file, one entry per shape.

SE-ARD, D = 6, P = 4 (the objective and C = 3 constraints are the model's outputs), var_add = the kernel's noise, terms and partials
asked for, for (N, candidates) in {(16384, 16384), (4096, 4096)}.  Per shape, in ONE process, each the median of 5 after a warm-up:

  fused        gpe_logcei_batch, host to host (time.perf_counter around the call; logcei, terms and partials read back), and its
               three phases (gpe_cei_phase_ms: the solves, the kernel, the read-back)
  query        gpe_query_batch alone, returning mu (M x 4) and var to the host: what the fused call adds the kernel to
  query+numpy  the route the library offered before: that gpe_query_batch, then tests/cei_ref.py's ref_logcei on the host
               `same_values`: the largest |fused - numpy| / max(1, |numpy|) over values, terms and partials

    python profiles/cei_timing.py [--shape 0|1] [--out profiles/cei_timing.json]      (an existing file is extended)
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(16384, 16384), (4096, 4096)]
REPS, D, C, NOISE = 5, 6, 3, 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", type=int, default=None)
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    from limbo_amd import _capi
    from tests import cei_ref as R

    eng = _capi.load_engine()
    out = {"what": f"SE-ARD D = {D}, P = {1 + C} (objective + {C} constraints), var_add = noise, with terms and partials; ms; host to host "
                   "unless a phase; medians of 5 after a warm-up", "shapes": {}}
    if a.out and Path(a.out).exists():
        out = json.loads(Path(a.out).read_text())
    for N, M in (SHAPES if a.shape is None else [SHAPES[a.shape]]):
        rng = np.random.default_rng(N + M)
        X, V = rng.random((N, D)), rng.random((M, D))
        Y = np.stack([np.sin(3.0 * X @ rng.random(D))] + [np.cos(3.0 * X @ rng.random(D)) for _ in range(C)], axis=1) + 0.1 * rng.standard_normal((N, 1 + C))
        om = Y - Y.mean(axis=0)
        thr = np.array([-0.2, 0.0, 0.2])
        f_best = float(np.sort(om[:, 0])[-10])
        h = _capi.Handle(eng)
        h.set_data(X, om)
        h.set_kernel(_capi.KERNEL_SE_ARD, np.log([0.3, 0.45, 0.6, 0.75, 0.9, 1.0, 1.0]), NOISE)
        assert h.compute() == 0
        h.set_profiling(True)
        t, phases = [], []
        for r in range(1 + REPS):  # (r = 0: the warm-up)
            t0 = time.perf_counter()
            rc, lc, tm, p, _, _ = h.logcei_batch(V, thr, [1, 2, 3], 0, f_best, 0.0, True, None, NOISE, want=("logcei", "terms", "partials"))
            dt = time.perf_counter() - t0
            assert rc == 0
            if r:
                t.append(dt * 1e3)
                phases.append(h.cei_phase_ms())
        ph = {k: float(np.median([q[k] for q in phases])) for k in phases[0]}
        rec = {"fused_ms": float(np.median(t)), "phases_ms": ph, "kernel_share_of_call": ph["kernel"] / float(np.median(t)),
               "candidates_per_s_in_kernel": M / (ph["kernel"] * 1e-3), "logcei_max": float(lc.max()), "logcei_median": float(np.median(lc)),
               "logcei_min": float(lc.min())}
        tq, ts = [], []
        for r in range(1 + REPS):
            t0 = time.perf_counter()
            kta, var = h.query_batch(V)
            t1 = time.perf_counter()
            sd = np.sqrt(np.where(var > np.finfo(float).eps, var, 0.0) + NOISE)
            val, terms, part = R.ref_logcei(1, f_best, 0.0, thr, kta[:, 0], sd, kta[:, 1:], np.tile(sd[:, None], (1, C)))
            t2 = time.perf_counter()
            if r:
                tq.append((t1 - t0) * 1e3)
                ts.append((t2 - t1) * 1e3)
        same = max(float(R.err(g, w).max()) for g, w in ((lc, val), (tm, terms), (p, part)))
        rec["query_batch_ms"] = float(np.median(tq))
        rec["query_plus_numpy"] = {"numpy_epilogue_ms": float(np.median(ts)), "total_ms": float(np.median(tq)) + float(np.median(ts)), "same_values": same}
        rec["fused_over_query_batch"] = rec["fused_ms"] / rec["query_batch_ms"]
        rec["speedup_over_query_plus_numpy"] = rec["query_plus_numpy"]["total_ms"] / rec["fused_ms"]
        out["shapes"][f"{N}x{M}xC{C}"] = rec
        h.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
