#!/usr/bin/env python
"""Timing of gpe_remove_samples (include/gpe_remove.h): the factor update against the recompute — one JSON line.

For N in {1024, 4096, 16384} and the patterns oldest 1, oldest 16, 16 at random, newest 16 — and 8 and 32 from index 0 at
N = 16384 — SE-ARD, D = 6, P = 1:
  update_ms     host-to-host time of ONE gpe_remove_samples with how = UPDATE,
  recompute_ms  the same with how = RECOMPUTE: K rebuilt on the remaining samples and factored, which is what a caller had before,
  auto_ms       the same with how = AUTO (the plan's choice: `plan`, from gpe_debug_remove_plan),
each the median of 5 after one warm-up, with the minimum and maximum of the 5, every repeat on a fresh clone of the same state.
That state holds a K^-1 (which every removal invalidates): the clones own the ld x cap slot the update writes into, so neither
side pays for an allocation, as in a running loop, where the slot stays with the handle after the first removal.
`spread` is the largest (max - min) / median of the three; `auto_excess` is auto_ms / min(update_ms, recompute_ms) - 1: AUTO is
acceptable where it does not exceed the spread.  A separate profiled UPDATE gives the per-phase split.

    python tools/remove_bench.py [--out profiles/remove_samples_timing.json] [--sizes 1024,4096]
"""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SIZES = [1024, 4096, 16384]
D = 6


def patterns(N, rng):
    p = {"oldest1": [0], "oldest16": list(range(16)), "random16": sorted(rng.choice(N, 16, replace=False).tolist()),
         "newest16": list(range(N - 16, N))}
    if N == 16384:
        p["oldest8"] = list(range(8))
        p["oldest32"] = list(range(32))
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default=None)
    a = ap.parse_args()
    import numpy as np

    sys.path.insert(0, str(ROOT))
    from limbo_amd import _capi

    sizes = SIZES if not a.sizes else [int(v) for v in a.sizes.split(",")]
    eng = _capi.load_engine()
    hbm = ctypes.c_double()
    assert eng.fn("hbm_stream_peak")(0, ctypes.byref(hbm)) == 0
    res = {"what": "gpe_remove_samples: UPDATE against RECOMPUTE against AUTO, SE-ARD D = 6 P = 1, fresh clone per repeat, ms",
           "max_vectors": _capi.remove_max_vectors(eng), "hbm_gbs": hbm.value, "shapes": {}}
    for N in sizes:
        rng = np.random.default_rng(N)
        X = rng.random((N, D))
        y = np.sin(3.0 * X @ rng.random(D)) + 0.05 * rng.standard_normal(N)
        base = _capi.Handle(eng)
        base.set_data(X, (y - y.mean())[:, None])
        base.set_kernel(_capi.KERNEL_SE_ARD, np.log([0.3, 0.45, 0.6, 0.75, 0.9, 1.0, 1.0]), 0.01)
        assert base.compute() == 0
        base.compute_inv_kernel()  # (the clones then own a K^-1 slot, the update's second matrix: no allocation inside the timed call)
        for name, R in patterns(N, rng).items():
            keep = np.ones(N, bool)
            keep[R] = False
            om = (y[keep] - y[keep].mean())[:, None]

            def timed(how, reps=5):
                ts = []
                for r in range(reps + 1):
                    h = base.clone()
                    t0 = time.perf_counter()
                    rc = h.remove_samples(R, om, how)
                    t1 = time.perf_counter()
                    assert rc == 0 and h.nb_samples() == N - len(R) and h.flow_retries() == 0
                    h.close()
                    if r > 0:
                        ts.append((t1 - t0) * 1e3)
                return {"ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}

            row = {"q": len(R), "i0": int(R[0]), "update": timed("update"), "recompute": timed("recompute"), "auto": timed("auto"),
                   "plan": _capi.debug_remove_plan(eng, N, R[0], len(R), R[0] == N - len(R))}
            row["spread"] = max((v["max_ms"] - v["min_ms"]) / v["ms"] for v in (row["update"], row["recompute"], row["auto"]))
            row["auto_excess"] = row["auto"]["ms"] / min(row["update"]["ms"], row["recompute"]["ms"]) - 1.0
            h = base.clone()
            h.set_profiling(True)
            h.reset_phase_ms()
            assert h.remove_samples(R, om, "update") == 0
            row["update_phases"] = {k: v for k, v in h.get_phase_ms().items() if v["launches"] > 0}
            h.close()
            ph = row["update_phases"].get("potrf_update")
            if ph and ph["ms"] > 0:  # the trailing part read once and written once
                m = N - R[0] // 256 * 256
                row["factor_of_hbm_peak"] = 16.0 * (m * (m + 1) / 2.0 + (N - m) * N) / (ph["ms"] * 1e-3) / (hbm.value * 1e9)
            res["shapes"][f"{N}:{name}"] = row
            print(f"{N}:{name}", {k: row[k] for k in ("update", "recompute", "auto", "plan")}, file=sys.stderr, flush=True)
        base.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
