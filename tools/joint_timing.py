#!/usr/bin/env python
"""Timing of the joint posterior (include/gpe_joint.h) — one JSON line.

For (N, M) in {(4096, 512), (4096, 2048), (16384, 1024), (16384, 4096)}, SE-ARD, D = 6: gpe_joint_draws with S = 16 (only the
arg-max leaves the device), median of 20 calls after 2 warm-ups, per phase — Z = L^-1 k(X, V), Sigma, its factorisation, the
draws — with the fraction of the fp64 matrix-core peak that the engine's own gpe_mfma_f64_peak reports, for both covariance
paths: the split kernel (GPE_JOINT_SPLITK=1) and the composed path (GPE_JOINT_SPLITK=0: kernel-matrix build on V, the
triangular update with k = N, the mirror).  The switch is read once per process, so every path runs in child processes of its
own, in the order split, composed, composed, split (the order reversed once): a drift of the device shows as a difference
between the two runs of a path.  A last child runs the engine's default dispatch; cov_verdict says which path that was.
`spread` is (max - min) / median of a run's 20 samples of the Sigma phase.

    python tools/joint_timing.py [--out profiles/joint_posterior_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(4096, 512), (4096, 2048), (16384, 1024), (16384, 4096)]
REPS, WARM, S, D = 20, 2, 16, 6


def child():
    import numpy as np

    sys.path.insert(0, str(ROOT))
    from limbo_amd import _capi

    eng = _capi.load_engine()
    import ctypes

    peak = ctypes.c_double()
    assert eng.fn("mfma_f64_peak")(0, ctypes.byref(peak)) == 0
    out = {"peak_tflops": peak.value, "shapes": {}}
    for N, M in SHAPES:
        rng = np.random.default_rng(N + M)
        X, V = rng.random((N, D)), rng.random((M, D))
        y = np.sin(3.0 * X @ rng.random(D))
        h = _capi.Handle(eng)
        h.set_data(X, y - y.mean())
        h.set_kernel(_capi.KERNEL_SE_ARD, np.log([0.3, 0.45, 0.6, 0.75, 0.9, 1.0, 1.0]), 0.01)
        assert h.compute() == 0
        Z = rng.standard_normal((M, S, 1))
        h.set_profiling(True)
        rows = []
        for r in range(WARM + REPS):
            rc, _, am, _ = h.joint_draws(V, Z, 1e-6, want_F=False)
            assert rc == 0
            if r >= WARM:
                rows.append(h.joint_phase_ms())
        assert h.flow_retries() == 0 and h.handover_reruns() == 0
        h.close()
        med = {k: float(np.median([q[k] for q in rows])) for k in rows[0]}
        cov = np.array([q["cov"] for q in rows])
        flops = {"Z": float(M) * N * N, "cov": float(M) * M * N, "chol": float(M) ** 3 / 3.0, "draws": float(M) * M * S}
        out["shapes"][f"{N}x{M}"] = {
            "ms": med,
            "of_peak": {k: flops[k] / (med[k] * 1e-3) / (peak.value * 1e12) for k in med if med[k] > 0},
            "cov_spread": float((cov.max() - cov.min()) / np.median(cov)),
            "cov_min_ms": float(cov.min()),
            "cov_max_ms": float(cov.max()),
        }
    print("JOINT_TIMING " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child()
    runs = []
    for path in ("split", "composed", "composed", "split", "default"):
        env = dict(os.environ)
        env.pop("GPE_JOINT_SPLITK", None)  # (default: the engine's own dispatch)
        if path != "default":
            env["GPE_JOINT_SPLITK"] = "1" if path == "split" else "0"
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child"], env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            return 1  # (a failed child ends the measurement: nothing more is started on the device)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("JOINT_TIMING ")][-1]
        runs.append({"path": path, **json.loads(line[len("JOINT_TIMING "):])})
    # the dispatch rule: the split kernel where it is faster than the composed path by more than that path's own spread
    verdict = {}
    for N, M in SHAPES:
        k = f"{N}x{M}"
        sp = [r["shapes"][k] for r in runs if r["path"] == "split"]
        co = [r["shapes"][k] for r in runs if r["path"] == "composed"]
        sp_ms = max(q["ms"]["cov"] for q in sp)  # (the slower of the split's two runs against the faster of the composed path's)
        co_ms = min(q["ms"]["cov"] for q in co)
        co_spread = max(q["cov_spread"] for q in co)
        de_ms = [r["shapes"][k]["ms"]["cov"] for r in runs if r["path"] == "default"][0]
        verdict[k] = {"split_ms": sp_ms, "composed_ms": co_ms, "composed_spread": co_spread, "split_wins": bool(sp_ms < co_ms * (1.0 - co_spread)),
                      "default_ms": de_ms, "default_is": "split" if abs(de_ms - sp_ms) < abs(de_ms - co_ms) else "composed"}
    res = {"what": "gpe_joint_draws, S = 16, SE-ARD D = 6, median of 20 after 2 warm-ups; ms per phase", "runs": runs, "cov_verdict": verdict}
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
