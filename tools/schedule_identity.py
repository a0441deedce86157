#!/usr/bin/env python3
"""Same launches, same bits: the launch sequence and the results of one evaluation, per branch of the factorisation's schedule
(limbo_amd/csrc/schedule.hpp: potrf_blocked and its stages).  Run it on two builds, on the same device, and diff the outputs:
a change of the host side of the schedule that is a refactor leaves every line as it was.

    python tools/schedule_identity.py [--root TREE] [--cases a,b,..] > out.txt

TREE is the checkout whose built limbo_amd package is measured (default: the one this file is in).  Every case runs in a fresh
child process with its own environment (the switches are read once per process), one after another, each under its own time
limit; the first child that fails ends the run.  A case calls compute() twice on one handle and prints one JSON line:
the (stream index, kernel, grid, block) sequence of the SECOND evaluation (gpe_trace / gpe_trace_dump), the sha256 of
tril(get_L()) and of get_alpha(), and the bits of log_lik().  D = 4, SE-ARD, noise 0.01.

The case `lifecycle` is about the handle's memory instead of the schedule: one handle through every event that allocates, grows,
drops or hands on a device buffer (lifecycle_steps); it prints the sha256 of every array returned and the bits of every scalar.
"""
import argparse
import hashlib
import json
import os
import re
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

# case: (N, P, environment, what it reaches)
CASES = {
    "a": (512, 1, {}, "one launch is the whole factorisation, generating K itself"),
    "b": (520, 2, {}, "one launch plus the two-launch ragged finish"),
    "c": (562, 1, {}, "ragged block wider than 40 columns: ragged update, then the panel code"),
    "d": (512, 1, {"GPE_TAIL_MAX": "256", "GPE_TALL": "256"}, "tall [0,256), one update, closing"),
    "e": (1300, 3, {"GPE_TAIL_MAX": "256", "GPE_TALL": "0"}, "four look-ahead panels in front of a closing launch, ragged, P = 3"),
    "f": (1700, 1, {"GPE_TAIL_MAX": "0"}, "panels to the end, ragged last panel"),
    "g": (1700, 1, {"GPE_TAIL_MAX": "0", "GPE_EARLY_BULK_TILES": "0"}, "the p_done release"),
    "h": (1700, 1, {"GPE_TAIL_MAX": "0", "GPE_PANEL256": "0"}, "fused steps"),
    "i": (1700, 1, {"GPE_TAIL_MAX": "0", "GPE_PANEL256": "0", "GPE_PANEL_HANDOVER": "0"}, "head copy"),
    "j": (520, 1, {"GPE_FUSE_PANEL": "0"}, "the three-launch step"),
    "k": (520, 1, {"GPE_FUSE_DIAG": "0", "GPE_STOP_EVENT": "0"}, "the marker-packet form"),
    "l": (520, 1, {"GPE_LOOKAHEAD": "0"}, "single stream"),
    "m": (520, 1, {"GPE_NBO": "192"}, "a panel width the block-inverse paths do not take"),
    "n": (520, 1, {"GPE_TAIL_GEN": "0"}, "K built in front of the one-launch factorisation"),
    "o": (520, 1, {"GPE_RAGGED_FINISH": "0"}, "ragged update, k_diag_full, panel code"),
    "p": (3584, 1, {}, "the default three launches"),
    "q": (3640, 1, {}, "the default three launches, ragged 56"),
    "r": (4608, 1, {}, "default look-ahead panels in front of the closing launch"),
    "s": (520, 1, {}, "profiling on: the !c->prof branches"),
    "t": (700, 1, {}, "a batch of 3 through batch_compute: the batched path"),
    # k and l at N = 520 are one data-flow launch whatever the panel switches say; the same switches where the panels run
    "u": (1700, 1, {"GPE_TAIL_MAX": "0", "GPE_FUSE_DIAG": "0"}, "next-panel update with its own stop event, no fused diagonal block"),
    "v": (1700, 1, {"GPE_TAIL_MAX": "0", "GPE_FUSE_DIAG": "0", "GPE_STOP_EVENT": "0"}, "the marker-packet form in the panels"),
    "w": (1700, 1, {"GPE_TAIL_MAX": "0", "GPE_LOOKAHEAD": "0"}, "single stream in the panels"),
}
CASES["lifecycle"] = (300, 2, {}, "one handle through set_data, grow, the query scratch's give-back, a change of P, clone and destroy")
D = 4
NOISE = 0.01
CHILD_TIMEOUT_S = 180
_TRACE_LINE = re.compile(r"^\s*\S+\s+\S+\s+(\d+)\s+(.+?)\s+grid=(\d+),(\d+),(\d+)\s+block=(\d+)\s*$")


def problem(np, N, P, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (N, D))
    Y = np.stack([np.sin(X @ rng.standard_normal(D)) + 0.05 * rng.standard_normal(N) for _ in range(P)], axis=1)
    return X, Y - Y.mean(axis=0)


def lifecycle_steps(np, lib, Handle, se_ard):
    """One handle (of `lib`: the engine, or the oracle behind the same binding) through the events that move device memory, in
    order; yields (label, array or scalar) for everything a call returns.  The consumer may look at the process between two
    steps (tests/test_gpu_configs.py reads the live-buffer count there)."""
    theta = 0.1 * np.arange(D + 1) - 0.2
    X, Y = problem(np, 330, 2, 2000)
    h = Handle(lib, 0)
    # 1. N = 300 in a capacity of 320; K^-1, the LOO value and its gradient (dLinv, dKinv, dInvS.., dLooS, dLooV, dGradPartial)
    h.set_data(X[:300], Y[:300])
    h.set_kernel(se_ard, theta, NOISE)
    yield "1.set_data", None
    assert h.compute() == 0
    yield "1.log_lik", h.log_lik()
    yield "1.Kinv", h.get_Kinv()
    yield "1.loo", h.log_loo_cv()
    yield "1.loo_grad", h.log_loo_cv_grad(False)
    # 2. 30 samples one by one: 321 crosses the capacity (a multiple of the 64-row block) and takes the grow
    for n in range(300, 330):
        assert h.add_sample(X[n], Y[: n + 1]) == 0
    yield "2.alpha", h.get_alpha()
    yield "2.log_lik", h.log_lik()
    # 3. what the grow dropped, again
    yield "3.Kinv", h.get_Kinv()
    yield "3.loo_grad", h.log_loo_cv_grad(False)
    # 4. a batch whose scratch exceeds 64 MiB (given back), then a handful of points (allocated again, small)
    Xq = np.random.default_rng(2001).uniform(-2.0, 2.0, (16384, D))
    kta, var = h.query_batch(Xq)
    yield "4.kta_16384", kta
    yield "4.var_16384", var
    kta, var = h.query_batch(Xq[:3])
    yield "4.kta_3", kta
    yield "4.var_3", var
    # 5. fewer samples but another P: everything anew
    X1, Y1 = problem(np, 700, 1, 2002)
    h.set_data(X1[:200], Y1[:200])
    assert h.compute() == 0
    yield "5.alpha", h.get_alpha()
    yield "5.log_lik", h.log_lik()
    # 6. more samples than the capacity
    h.set_data(X1, Y1)
    lik, grad, rc = h.hp_objective(se_ard, theta + 0.05, NOISE, False, True)
    assert rc == 0
    yield "6.lik", lik
    yield "6.grad", grad
    # 7. the clone outlives its source
    c = h.clone()
    h.close()
    assert c.compute() == 0
    yield "7.alpha", c.get_alpha()
    kta, var = c.query_batch(Xq[:1000])
    yield "7.kta", kta
    yield "7.var", var
    c.close()


def run_lifecycle(np, _capi):
    import numbers

    out = {"case": "lifecycle"}
    for label, v in lifecycle_steps(np, _capi.load_engine(), _capi.Handle, _capi.KERNEL_SE_ARD):
        if v is None:
            continue
        if isinstance(v, numbers.Real):
            out[label + "_bits"] = struct.pack(">d", v).hex()
        else:
            out[label + "_sha256"] = hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()
    print(json.dumps(out), flush=True)


def run_case(name, root):
    sys.path.insert(0, str(root))
    import numpy as np

    from limbo_amd import _capi

    assert Path(_capi.__file__).resolve().is_relative_to(root), _capi.__file__
    if name == "lifecycle":
        return run_lifecycle(np, _capi)
    N, P, _, _ = CASES[name]
    lib = _capi.load_engine()
    hs = []
    for g in range(3 if name == "t" else 1):
        h = _capi.Handle(lib, 0)
        h.set_data(*problem(np, N, P, 1000 + g))
        h.set_kernel(_capi.KERNEL_SE_ARD, 0.1 * np.arange(D + 1) - 0.2, NOISE)
        if name == "s":
            h.set_profiling(True)
        hs.append(h)

    def evaluate():
        st = _capi.batch_compute(hs) if name == "t" else [hs[0].compute()]
        assert all(s == 0 for s in st), st

    evaluate()
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "trace.txt"
        try:
            assert lib.fn("trace")(1) == 0
            evaluate()
            assert lib.fn("trace_dump")(str(path).encode()) == 0
        finally:
            lib.fn("trace")(0)
        lines = path.read_text().splitlines()
    recs = [_TRACE_LINE.match(ln) for ln in lines]
    assert lines and all(recs), lines[:3]
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    out = {
        "case": name,
        "N": N,
        "P": P,
        "launches": [[int(m[1]), m[2], [int(m[3]), int(m[4]), int(m[5])], int(m[6])] for m in recs],
        "L_sha256": [sha(np.tril(h.get_L())) for h in hs],
        "alpha_sha256": [sha(h.get_alpha()) for h in hs],
        "log_lik_bits": [struct.pack(">d", h.log_lik()).hex() for h in hs],
    }
    for h in hs:
        h.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent))
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    root = Path(a.root).resolve()
    if a.child:
        run_case(a.child, root)
        return 0
    for name in a.cases.split(","):
        env = {k: v for k, v in os.environ.items() if not k.startswith("GPE_")}
        env.update(CASES[name][2])
        try:
            rc = subprocess.run([sys.executable, __file__, "--root", str(root), "--child", name], env=env, timeout=CHILD_TIMEOUT_S).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"case {name}: the child ended with status {rc}; stopping", file=sys.stderr)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
