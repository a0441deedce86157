#!/usr/bin/env python
"""Timing of greedy batch selection (include/gpe_batch_select.h) — one JSON line.

SE-ARD, D = 6, P = 1, q = 16, the UCB rule (beta = 2, var_add = obs_noise = the noise), for (N, M) in {(4096, 4096), (16384, 1024),
(16384, 16384)}.  Per shape, in ONE process and alternating call by call (a drift of the device hits every path alike):

  select      gpe_select_batch, host to host (time.perf_counter around the call), median of 10 after a warm-up, and its three
              phases (gpe_select_phase_ms: setup = Zt + kta + var_0, the 16 rounds, the read-back).  `hbm_share` = q M N 8 bytes
              over the rounds phase against the 6.29 TB/s a float4 copy reaches on this chip: what the column product gets, with
              the gather, fold and pick launches of every round counted against it.
  composed    what the library offered for the same answer before: gpe_joint_query returning Sigma to the host and the recursion
              in numpy on it (`same_picks`: whether its batch is select's).
  draws       gpe_joint_draws with S = 16 (only the arg-max leaves the device): the random alternative, for context.

A path that cannot run at a shape (Sigma's scratch) is recorded with the reason instead of a time.

    python tools/batch_select_timing.py [--out profiles/batch_select_timing.json]
"""
import argparse
import json
import math
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(4096, 4096), (16384, 1024), (16384, 16384)]
REPS, Q, D, S, BETA, NOISE = 10, 16, 6, 16, 2.0, 0.01
COPY_RATE = 6.29e12  # bytes/s, measured float4 copy


def recursion(Sig, mu, q, beta, var_add, lam):
    """the header's recursion (UCB, distinct) in numpy on a full covariance"""
    var = np.diag(Sig).copy()
    W = np.zeros((len(mu), q))
    idx = []
    for t in range(q):
        s = mu + beta * np.sqrt(np.where(var <= np.finfo(float).eps, 0.0, var) + var_add)
        s[idx] = -np.inf
        j = int(np.argmax(s))
        idx.append(j)
        c = Sig[:, j] - W[:, :t] @ W[j, :t]
        W[:, t] = c / math.sqrt(c[j] + lam)
        var -= W[:, t] ** 2
    return np.array(idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    from limbo_amd import _capi

    eng = _capi.load_engine()
    out = {"what": f"SE-ARD D = {D}, P = 1, q = {Q}, UCB; ms, median of {REPS} alternating calls after a warm-up; host to host unless a phase",
           "copy_rate_TBps": COPY_RATE / 1e12, "shapes": {}}
    for N, M in SHAPES:
        rng = np.random.default_rng(N + M)
        X, V = rng.random((N, D)), rng.random((M, D))
        y = np.sin(3.0 * X @ rng.random(D))
        h = _capi.Handle(eng)
        h.set_data(X, y - y.mean())
        h.set_kernel(_capi.KERNEL_SE_ARD, np.log([0.3, 0.45, 0.6, 0.75, 0.9, 1.0, 1.0]), NOISE)
        assert h.compute() == 0
        h.set_profiling(True)
        Z = rng.standard_normal((M, S, 1))
        reps = {"select": REPS, "composed": REPS if M <= 4096 else 3, "draws": REPS if M <= 4096 else 3}
        t = {k: [] for k in reps}
        phases, left_out, picks = [], {}, {}
        for r in range(1 + REPS):  # (r = 0: the warm-up of every path)
            t0 = time.perf_counter()
            rc, idx, _, _, _ = h.select_batch(V, Q, _capi.SELECT_UCB, BETA, var_add=NOISE, obs_noise=NOISE, want=("idx", "score"))
            dt = time.perf_counter() - t0
            assert rc == 0
            picks["select"] = idx
            if r:
                t["select"].append(dt * 1e3)
                phases.append(h.select_phase_ms())
            for path in ("composed", "draws"):
                if path in left_out or r > reps[path]:
                    continue
                try:
                    t0 = time.perf_counter()
                    if path == "composed":
                        kta, cov = h.joint_query(V, 0.0)
                        picks["composed"] = recursion(cov, kta[:, 0], Q, BETA, NOISE, NOISE)
                        del cov
                    else:
                        assert h.joint_draws(V, Z, 1e-6, want_F=False)[0] == 0
                    dt = time.perf_counter() - t0
                    if r:
                        t[path].append(dt * 1e3)
                except (_capi.EngineError, MemoryError) as e:
                    left_out[path] = str(e)[:200]
        assert h.flow_retries() == 0 and h.handover_reruns() == 0
        h.close()
        med = {k: float(np.median(v)) for k, v in t.items() if v}
        ph = {k: float(np.median([p[k] for p in phases])) for k in phases[0]}
        row = {"ms": med, "reps": {k: len(v) for k, v in t.items()}, "select_phase_ms": ph, "left_out": left_out,
               "min_max_ms": {k: [float(min(v)), float(max(v))] for k, v in t.items() if v},
               "same_picks": bool(np.array_equal(picks["composed"], picks["select"])) if "composed" in picks else None,
               "rounds_bytes": Q * M * N * 8, "hbm_share": Q * M * N * 8 / (ph["rounds"] * 1e-3) / COPY_RATE}
        for k in ("composed", "draws"):
            if k in med:
                row[k + "_over_select"] = med[k] / med["select"]
        out["shapes"][f"{N}x{M}"] = row
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
