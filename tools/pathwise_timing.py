#!/usr/bin/env python
"""Timing of pathwise posterior draws (include/gpe_pathwise.h) — one JSON line.

For N in {1024, 4096, 16384} and T in {4096, 16384, 262144}, SE-ARD, D = 6, P = 1, S = 16 draws on R = 2048 features: gpe_paths_create,
gpe_paths_eval (F alone; F and dF for T <= 16384) and gpe_paths_argmax, host to host (host clock around calls that end in a stream
wait), median of 10 after 2 warm-ups (T = 262144: median of 5 after 1, a call there takes seconds), with the phases of
gpe_paths_phase_ms from the last call.  Baselines in the same process on the same handle, for T <= 16384: gpe_joint_draws at M = T,
S = 16 (the way to a Thompson draw without paths) and gpe_query_batch_grad at M = T (the way to a gradient).  `model_gflop`: the
flop model of DESIGN §3.16 — paths 2 T N S (1 + D with the gradient) + 2 T R S (1 + D), joint M N^2 + M^2 N + M^3 / 3;
`data_tflops`: the data term's rate from its phase, `of_f64_peak` against gpe_mfma_f64_peak.

    python tools/pathwise_timing.py [--out profiles/pathwise_timing.json] [--quick]
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NS, TS, D, S, R = (1024, 4096, 16384), (4096, 16384, 262144), 6, 16, 2048


def timed(fn, reps, warm):
    ts = []
    for r in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        if r >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], (ts[-1] - ts[0]) / ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="N = 1024 and T = 4096 only (a check of the script)")
    a = ap.parse_args()
    import numpy as np

    sys.path.insert(0, str(ROOT))
    from limbo_amd import _capi

    eng = _capi.load_engine()
    peak, hbm = C.c_double(0), C.c_double(0)
    eng.fn("mfma_f64_peak")(0, C.byref(peak))
    eng.fn("hbm_stream_peak")(0, C.byref(hbm))
    shapes = {}
    for N in (NS[:1] if a.quick else NS):
        rng = np.random.default_rng(N)
        X = rng.random((N, D))
        y = np.sin(3.0 * X @ rng.random(D)) + 0.1 * rng.standard_normal(N)
        h = _capi.Handle(eng)
        h.set_data(X, y - y.mean())
        h.set_kernel(_capi.KERNEL_SE_ARD, np.log([0.3, 0.45, 0.6, 0.75, 0.9, 1.0, 1.0]), 0.01)
        assert h.compute() == 0
        Om, ph = rng.standard_normal((R, D)), rng.uniform(0, 2 * np.pi, R)
        W, E = rng.standard_normal((R, S, 1)), rng.standard_normal((N, S, 1))
        made = []

        def create():
            if made:
                made.pop().close()
            made.append(h.paths(R, S, Om, ph, W, E))

        create_ms, create_spread = timed(create, 10, 2)
        ps = made[0]
        create_ph = ps.phase_ms()
        for T in (TS[:1] if a.quick else TS):
            V = rng.random((T, D))
            reps, warm = (5, 1) if T > 16384 else (10, 2)
            row = {"create_ms": create_ms, "create_spread": create_spread,
                   "create_phase_ms": {k: create_ph[k] for k in ("create_features", "create_solve")}, "reps": reps}
            row["eval_F_ms"], row["eval_F_spread"] = timed(lambda: ps.eval(V, want=("F",)), reps, warm)
            p = ps.phase_ms()
            row["eval_F_phase_ms"] = {"features": p["eval_features"], "data": p["eval_data"]}
            row["data_tflops_F"] = 2.0 * T * N * S / (p["eval_data"] * 1e-3) / 1e12
            row["argmax_ms"], row["argmax_spread"] = timed(lambda: ps.argmax(V), reps, warm)
            row["model_gflop"] = {"paths_F": (2.0 * T * N * S + 2.0 * T * R * S) / 1e9}
            if T <= 16384:
                row["eval_FdF_ms"], row["eval_FdF_spread"] = timed(lambda: ps.eval(V), reps, warm)
                p = ps.phase_ms()
                row["eval_FdF_phase_ms"] = {"features": p["eval_features"], "data": p["eval_data"]}
                row["data_tflops_FdF"] = 2.0 * T * N * S * (1 + D) / (p["eval_data"] * 1e-3) / 1e12
                Z = rng.standard_normal((T, S, 1))
                row["joint_draws_ms"], row["joint_draws_spread"] = timed(lambda: h.joint_draws(V, Z, 1e-6, want_F=False), reps, warm)
                row["query_batch_grad_ms"], row["query_batch_grad_spread"] = timed(lambda: h.query_batch_grad(V), reps, warm)
                row["model_gflop"].update({"paths_FdF": (2.0 * T * N * S + 2.0 * T * R * S) * (1 + D) / 1e9,
                                           "joint": (float(T) * N * N + float(T) * T * N + float(T) ** 3 / 3.0) / 1e9})
                row["argmax_vs_joint"] = row["argmax_ms"] / row["joint_draws_ms"]
                row["FdF_vs_query_grad"] = row["eval_FdF_ms"] / row["query_batch_grad_ms"]
            if peak.value > 0:
                row["of_f64_peak"] = {k[12:]: row[k] / peak.value for k in ("data_tflops_F", "data_tflops_FdF") if k in row}
            shapes[f"{N}x{T}"] = row
            print(f"{N}x{T}", json.dumps(row), file=sys.stderr, flush=True)
        ps.close()
        h.close()
    res = {"what": "pathwise draws, SE-ARD D = 6 P = 1, S = 16, R = 2048; host to host, host clock, median of `reps` after 2 (1) warm-ups; "
                   "baselines gpe_joint_draws (arg-max only, jitter 1e-6) and gpe_query_batch_grad at M = T in the same process",
           "mfma_f64_peak_tflops": peak.value, "hbm_stream_peak_gbs": hbm.value, "shapes": shapes}
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
