#!/usr/bin/env python
"""Timing of the knowledge gradient over a finite alternative set (include/gpe_kg.h) — one JSON file, one entry per shape.

SE-ARD, D = 6, P = 1, with_self = 1, obs_noise = the kernel's noise, for (N, A, M) in {(16384, 1024, 16384), (4096, 512, 4096)}.
Per shape, in ONE process:

  kg          gpe_kg_batch, host to host (time.perf_counter around the call, kg alone read back), median of 5 after a warm-up, and
              its four phases (gpe_kg_phase_ms: the alternatives' pass, the candidates' solves with the cross-covariance, the
              envelopes, the read-back).  `pair_steps_per_s` = M (A + 1)^2 over the envelope phase.
  baseline    what the library offered for the same answer before: gpe_joint_query on the concatenated batch returning Sigma to the
              host (median of 3), and the envelope in numpy on it (tests/kg_ref.py, timed on `env_sample` candidates and scaled to all
              of them: `envelope_ms_scaled`).  Where A + M exceeds gpe_joint_max_points the baseline takes the largest M that fits
              (`M_baseline`) — it cannot serve the shape at all.  `same_values`: the largest relative difference between the two
              routes on the sampled candidates.

    python tools/kg_timing.py [--shape 0|1] [--out profiles/kg_timing.json]      (an existing file is extended)
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(16384, 1024, 16384), (4096, 512, 4096)]
REPS, D, NOISE, ENV_SAMPLE = 5, 6, 0.01, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", type=int, default=None)
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    from limbo_amd import _capi
    from tests import kg_ref as R

    eng = _capi.load_engine()
    out = {"what": f"SE-ARD D = {D}, P = 1, with_self = 1; ms; host to host unless a phase", "shapes": {}}
    if a.out and Path(a.out).exists():
        out = json.loads(Path(a.out).read_text())
    for N, A, M in (SHAPES if a.shape is None else [SHAPES[a.shape]]):
        rng = np.random.default_rng(N + A + M)
        X, Va, Vc = rng.random((N, D)), rng.random((A, D)), rng.random((M, D))
        y = np.sin(3.0 * X @ rng.random(D)) + 0.1 * rng.standard_normal(N)
        h = _capi.Handle(eng)
        h.set_data(X, y - y.mean())
        h.set_kernel(_capi.KERNEL_SE_ARD, np.log([0.3, 0.45, 0.6, 0.75, 0.9, 1.0, 1.0]), NOISE)
        assert h.compute() == 0
        h.set_profiling(True)
        t, phases = [], []
        for r in range(1 + REPS):  # (r = 0: the warm-up)
            t0 = time.perf_counter()
            rc, kg, _, _ = h.kg_batch(Va, Vc, NOISE, True, want=("kg",))
            dt = time.perf_counter() - t0
            assert rc == 0
            if r:
                t.append(dt * 1e3)
                phases.append(h.kg_phase_ms())
        ph = {k: float(np.median([p[k] for p in phases])) for k in phases[0]}
        rec = {"kg_ms": float(np.median(t)), "phases_ms": ph, "pair_steps_per_s": M * (A + 1.0) ** 2 / (ph["envelope"] * 1e-3),
               "kg_max": float(kg.max()), "kg_median": float(np.median(kg))}
        # the baseline: Sigma of the concatenated batch to the host, the envelope there
        Mb = min(M, h.joint_max_points() - A)
        V = np.vstack([Va, Vc[:Mb]])
        tj = []
        for r in range(1 + 3):
            t0 = time.perf_counter()
            kta, cov = h.joint_query(V, 0.0)
            if r:
                tj.append((time.perf_counter() - t0) * 1e3)
        sample = np.linspace(0, Mb - 1, ENV_SAMPLE).astype(int)
        t0 = time.perf_counter()
        ref = R.ref_kg(cov, kta[:, 0], np.arange(A), A + sample, NOISE, True)
        te = (time.perf_counter() - t0) * 1e3
        big = ref >= 1e-280
        rec["baseline"] = {"M_baseline": int(Mb), "note": "" if Mb == M else f"A + M exceeds gpe_joint_max_points = {A + Mb}: the largest M that fits",
                           "joint_query_ms": float(np.median(tj)), "sigma_bytes": int(cov.nbytes), "env_sample": ENV_SAMPLE,
                           "envelope_ms_scaled": te / ENV_SAMPLE * Mb,
                           "same_values": float(np.max(np.abs(kg[sample][big] - ref[big]) / ref[big])) if big.any() else 0.0}
        rec["baseline"]["total_ms"] = rec["baseline"]["joint_query_ms"] + rec["baseline"]["envelope_ms_scaled"]
        out["shapes"][f"{N}x{A}x{M}"] = rec
        h.close()
        del cov
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
