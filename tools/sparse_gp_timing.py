#!/usr/bin/env python
"""Timing of the sparse pseudo-input GP (include/gpe_sparse.h) — one JSON line.

For N in {131 072, 1 048 576}, D = 6, M in {512, 1024, 2048}: gpe_sp_compute phase by phase (K_mn and V, ep and r, the Gram, the
factorisation of A with bet; gpe_sp_phase_ms under profiling) and 10 000 predictions, median of REPS calls after one warm-up, for
both Gram paths — the split-k matrix-core kernel k_sp_gram (GPE_SPARSE_GRAM=1) and the composed path (GPE_SPARSE_GRAM=0: a weighted copy
of V through launch_gemm_sub with a_kmajor = b_kmajor = 1, overwrite = 2) — in the order kernel, composed, composed, kernel, so that
a drift of the device shows as a difference between the two runs of a path (the switch is read per call).  The Gram and the
solve are N M^2 flop each (the Gram: the lower triangle of 2 N M^2); of_peak is against the engine's own gpe_mfma_f64_peak.  The
dense engine's gpe_compute at N = 16 384 (its largest measured order) stands beside them for scale.

    python tools/sparse_gp_timing.py [--out profiles/sparse_gp_timing.json] [--quick]
"""
import argparse
import ctypes
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from limbo_amd import _capi  # noqa: E402

NS, MS, D, T, REPS = [131072, 1048576], [512, 1024, 2048], 6, 10000, 5
ELL = np.array([0.3, 0.45, 0.6, 0.75, 0.9, 1.0])


def run_path(h, Xt, gram):
    os.environ["GPE_SPARSE_GRAM"] = "1" if gram == "kernel" else "0"
    rows = []
    for r in range(1 + REPS):
        t0 = time.perf_counter()
        assert h.compute() == 0
        wall = (time.perf_counter() - t0) * 1e3
        h.predict(Xt)
        ph = h.phase_ms()
        ph["compute_wall"] = wall
        if r >= 1:
            rows.append(ph)
    os.environ.pop("GPE_SPARSE_GRAM", None)
    med = {k: float(np.median([q[k] for q in rows])) for k in rows[0]}
    g = np.array([q["gram"] for q in rows])
    return med, float((g.max() - g.min()) / np.median(g)), h.nlml().tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="N = 131 072 only")
    a = ap.parse_args()
    eng = _capi.load_engine()
    peak = ctypes.c_double()
    assert eng.fn("mfma_f64_peak")(0, ctypes.byref(peak)) == 0
    res = {"what": f"gpe_sp_compute per phase and {T} predictions, SE-ARD D = {D}, c = 1, sig = 0.01, jitter 1e-6; median of {REPS} after 1 warm-up; ms",
           "peak_tflops": peak.value, "shapes": {}}
    for N in (NS[:1] if a.quick else NS):
        rng = np.random.default_rng(N)
        X = rng.random((N, D))
        y = np.sin(3.0 * X @ rng.random(D)) + 0.1 * rng.standard_normal(N)
        y -= y.mean()
        Xt = rng.random((T, D))
        for M in MS:
            h = _capi.SparseHandle(eng)
            h.set_data(X, y)
            h.set_pseudo(X[rng.permutation(N)[:M]])
            h.set_hparams(-2.0 * np.log(ELL), 0.0, np.log(0.01), 1e-6)
            h.set_profiling(True)
            runs = []
            for gram in ("kernel", "composed", "composed", "kernel"):
                med, spread, nlml = run_path(h, Xt, gram)
                fl = float(N) * M * M
                runs.append({"gram": gram, "ms": med, "gram_spread": spread, "nlml": nlml,
                             "gram_tflops": fl / (med["gram"] * 1e-3) / 1e12, "gram_of_peak": fl / (med["gram"] * 1e-3) / (peak.value * 1e12),
                             "solve_of_peak": fl / (med["kmn_v"] * 1e-3) / (peak.value * 1e12)})
            h.close()
            ke = max(r["ms"]["gram"] for r in runs if r["gram"] == "kernel")  # the slower of the kernel's runs against the faster composed one
            co = min(r["ms"]["gram"] for r in runs if r["gram"] == "composed")
            res["shapes"][f"{N}x{M}"] = {"runs": runs,
                                         "verdict": {"kernel_ms": ke, "composed_ms": co, "kernel_wins": bool(ke < co)}}
            print(f"{N}x{M}: gram kernel {ke:.3f} ms, composed {co:.3f} ms", file=sys.stderr)
    # for scale: the exact model at the largest order the engine has been measured at
    N = 16384
    rng = np.random.default_rng(1)
    X = rng.random((N, D))
    y = np.sin(3.0 * X @ rng.random(D))
    d = _capi.Handle(eng)
    d.set_data(X, y - y.mean())
    d.set_kernel(_capi.KERNEL_SE_ARD, np.log(np.r_[ELL, 1.0]), 0.01)
    ts = []
    for r in range(4):
        t0 = time.perf_counter()
        assert d.compute() == 0
        ts.append((time.perf_counter() - t0) * 1e3)
    assert d.flow_retries() == 0 and d.handover_reruns() == 0
    d.close()
    res["dense_compute_n16384_ms"] = float(np.median(ts[1:]))
    k = "1048576x1024" if not a.quick else "131072x1024"
    res["faster_at_m1024"] = "kernel" if res["shapes"][k]["verdict"]["kernel_wins"] else "composed"
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
