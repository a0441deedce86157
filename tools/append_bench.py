#!/usr/bin/env python
"""Timing of the blocked append (include/gpe_append.h) against the add_sample loop — one JSON line.

For (N, q) in {(1024, 16), (4096, 64), (16384, 64), (16384, 1024)}, SE-ARD, D = 6, P = 1:
  batch_ms   host-to-host time of ONE gpe_add_samples of q points, median of 5 after one warm-up;
  loop_ms    the same q points through q successive gpe_add_sample calls (gpe_add_sample's launches are untouched by the
             batched call: this IS the loop a caller had before), median of 3 after one warm-up;
every repeat on a fresh clone of the same state.  That state has spare capacity (it was fitted on N - 1 samples and took one
add_sample, which doubled the buffers): neither side pays for the reallocation, as in a running loop.
A separate profiled call gives the per-phase split (gpe_get_phase_ms) and two roofline fractions: the solve Zt = Kst L^-T against
the fp64 matrix-core peak the engine's own gpe_mfma_f64_peak reports (the flops the query phase accounted for), and alpha's two
sweeps (2 x the lower triangle of L, 8 bytes an entry) against gpe_hbm_stream_peak.

    python tools/append_bench.py [--out profiles/add_samples_timing.json] [--shapes 1024x16,4096x64]
"""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(1024, 16), (4096, 64), (16384, 64), (16384, 1024)]
D = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None)
    a = ap.parse_args()
    import numpy as np

    sys.path.insert(0, str(ROOT))
    from limbo_amd import _capi

    shapes = SHAPES if not a.shapes else [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    eng = _capi.load_engine()
    peak, hbm = ctypes.c_double(), ctypes.c_double()
    assert eng.fn("mfma_f64_peak")(0, ctypes.byref(peak)) == 0
    assert eng.fn("hbm_stream_peak")(0, ctypes.byref(hbm)) == 0
    res = {"what": "gpe_add_samples against q gpe_add_sample calls, SE-ARD D = 6 P = 1, fresh clone per repeat, ms",
           "chunk": _capi.append_max_chunk(eng), "peak_tflops": peak.value, "hbm_gbs": hbm.value, "shapes": {}}
    for N, q in shapes:
        rng = np.random.default_rng(N + q)
        X = rng.random((N + q, D))
        y = np.sin(3.0 * X @ rng.random(D)) + 0.05 * rng.standard_normal(N + q)
        om = (y - y.mean())[:, None]
        base = _capi.Handle(eng)
        base.set_data(X[:N - 1], om[:N - 1])
        base.set_kernel(_capi.KERNEL_SE_ARD, np.log([0.3, 0.45, 0.6, 0.75, 0.9, 1.0, 1.0]), 0.01)
        assert base.compute() == 0
        assert base.add_sample(X[N - 1], om[:N]) == 0  # (the buffers double here, once)

        def batch(h):
            return h.add_samples(X[N:], om)

        def loop(h):
            rc = 0
            for i in range(N, N + q):
                rc |= h.add_sample(X[i], om[:i + 1])
            return rc

        def timed(fn, reps):
            ts = []
            for r in range(reps + 1):
                h = base.clone()
                t0 = time.perf_counter()
                rc = fn(h)
                t1 = time.perf_counter()
                assert rc == 0 and h.nb_samples() == N + q and h.flow_retries() == 0
                h.close()
                if r > 0:
                    ts.append((t1 - t0) * 1e3)
            return float(np.median(ts)), float(min(ts)), float(max(ts))

        b_med, b_min, b_max = timed(batch, 5)
        l_med, l_min, l_max = timed(loop, 3)
        h = base.clone()
        h.set_profiling(True)
        h.reset_phase_ms()
        assert batch(h) == 0
        ph = {k: v for k, v in h.get_phase_ms().items() if v["launches"] > 0}
        h.close()
        base.close()
        row = {"batch_ms": b_med, "batch_min_ms": b_min, "batch_max_ms": b_max, "loop_ms": l_med, "loop_min_ms": l_min, "loop_max_ms": l_max,
               "loop_over_batch": l_med / b_med, "phases": ph}
        if "query" in ph and ph["query"]["ms"] > 0:
            row["solve_of_mfma_peak"] = ph["query"]["flops"] / (ph["query"]["ms"] * 1e-3) / (peak.value * 1e12)
        if "solve" in ph and ph["solve"]["ms"] > 0:
            n1 = N + q
            row["alpha_of_hbm_peak"] = 2.0 * 8.0 * n1 * (n1 + 1) / 2.0 / (ph["solve"]["ms"] * 1e-3) / (hbm.value * 1e9)
        res["shapes"][f"{N}x{q}"] = row
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
