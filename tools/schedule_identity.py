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

The cases of QUERY_CASES and SPARSE_CASES are about the host side of the query family (limbo_amd/csrc/query.hpp and the calls
built on its chunk helpers): one line per call with its launches and the sha256 of every array it returned.

The cases of ACQ_CASES are about the host side of the acquisition family (limbo_amd/csrc/acq.hpp and the five calls built on it):
one line per call, as the query cases.

The case `shell` is about the handle's shell (limbo_amd/csrc/shell_layout.h: the streams, the device block and the pinned block
that a destroyed handle leaves to the next one): three handles in a row in one process, each taking the shell of the one before,
through every region of the two blocks (run_shell_case); one line per call, as the query cases.
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
    "h": (1700, 1, {"GPE_TAIL_MAX": "0", "GPE_PANEL256": "0"}, "fused steps"),
    "i": (1700, 1, {"GPE_TAIL_MAX": "0", "GPE_PANEL256": "0", "GPE_PANEL_HANDOVER": "0"}, "head copy"),
    "j": (520, 1, {"GPE_FUSE_PANEL": "0"}, "the three-launch step"),
    "k": (520, 1, {"GPE_FUSE_DIAG": "0", "GPE_STOP_EVENT": "0"}, "the marker-packet form"),
    "l": (520, 1, {"GPE_LOOKAHEAD": "0"}, "single stream"),
    "n": (520, 1, {"GPE_TAIL_GEN": "0"}, "K built in front of the one-launch factorisation"),
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
# The query family (limbo_amd/csrc/query.hpp and the calls built on its chunk helpers): a fitted model (P = 2) through query_batch,
# query_batch_cross, query_batch_grad, joint_query, joint_draws, a path set, add_samples + a query.  One line per call: its
# launches and the sha256 of every array it returned.  case: (N, points, Lambda columns, profiling, environment, what it reaches)
QUERY_CASES = {
    "q64": (520, 70, 0, False, {}, "the transposed layout, 64-tiles, ragged in N and in the points"),
    "q128": (1100, 70, 0, False, {}, "the transposed layout, 128-tiles"),
    "qnm": (520, 70, 0, False, {"GPE_QUERY_T": "0"}, "N x M by the switch; the joint posterior stays transposed"),
    "qsub": (200, 70, 0, False, {"GPE_SMALL": "0"}, "fewer samples than one outer panel: N x M"),
    "qfew": (520, 5, 0, False, {}, "a handful of points: the one-launch sweep of query_impl"),
    "qlam": (520, 70, 1, False, {}, "SE-ARD with one Lambda column: project_lambda launches"),
    "qprof": (520, 70, 0, True, {}, "profiling on: the timers' branches"),
    "qprofnm": (520, 70, 0, True, {"GPE_QUERY_T": "0"}, "profiling on in the N x M layout"),
}
# The sparse model: sp_compute, sp_predict, sp_grad, with sp_set_profiling off and on (the *_phase_ms values are times: printed as
# "finite and >= 0" only).  case: (N, pseudo-inputs, points, environment, what it reaches)
SPARSE_CASES = {
    "s130": (1300, 130, 130, {}, "fewer pseudo-inputs than one outer panel: N x M, one chunk"),
    "s130c": (1300, 130, 130, {"GPE_SPARSE_CHUNK": "512"}, "... three chunks, ragged last"),
    "s300": (1300, 300, 130, {}, "the transposed layout: both panel solves of the prediction"),
    "s300c": (1300, 300, 130, {"GPE_SPARSE_CHUNK": "512", "GPE_QUERY_T": "0"}, "... three chunks; transposed whatever GPE_QUERY_T says"),
}
# The acquisition family (limbo_amd/csrc/acq.hpp: kg, ehvi, cei, mes, nei): a fitted model (P = 4) through every fused call — with
# everything wanted and with a strict subset, with and without the caller's means — and every call on host-supplied beliefs.
# case: (N, candidates, profiling, environment, what it reaches)
ACQ_CASES = {
    "a520": (520, 70, False, {}, "the transposed layout"),
    "a200": (200, 70, False, {}, "fewer samples than one outer panel: N x M"),
    "a200x": (200, 8192 + 65, False, {}, "N x M, the fused calls' loop twice"),
    "aprof": (520, 70, True, {}, "profiling on: the timers' branches"),
    "aprofnm": (200, 70, True, {}, "profiling on in the N x M layout"),
}
SHELL_CASES = {"shell": ({}, "three handles on one pooled shell: stepped panels with head copy, one-launch panels, the small path")}
ALL_CASES = {**CASES, **QUERY_CASES, **SPARSE_CASES, **ACQ_CASES, **SHELL_CASES}
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


def traced(lib, call):
    """(what `call` returned, the launches it made: [stream index, kernel, grid, block] each)"""
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "trace.txt"
        try:
            assert lib.fn("trace")(1) == 0
            res = call()
            assert lib.fn("trace_dump")(str(path).encode()) == 0
        finally:
            lib.fn("trace")(0)
        lines = path.read_text().splitlines()
    recs = [_TRACE_LINE.match(ln) for ln in lines]
    assert lines and all(recs), lines[:3]
    return res, [[int(m[1]), m[2], [int(m[3]), int(m[4]), int(m[5])], int(m[6])] for m in recs]


def report(np, case, label, launches, arrays, times=None):
    """one line: a call's launches, the sha256 of its arrays (None: not asked for) and — times — whether they are finite and >= 0"""
    sha = lambda a: None if a is None else hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    out = {"case": case, "call": label, "launches": launches, "sha256": {k: sha(v) for k, v in arrays.items()}}
    if times is not None:
        out["times_finite_nonneg"] = {k: bool(np.isfinite(v) and v >= 0.0) for k, v in times.items()}
    print(json.dumps(out), flush=True)


def run_query_case(np, _capi, name):
    N, M, lam, prof, _, _ = QUERY_CASES[name]
    P, S, R, q_new = 2, 3, 64, 40
    lib = _capi.load_engine()
    X, Y = problem(np, N + q_new, P, 3000)
    rng = np.random.default_rng(3001)
    Xq = rng.uniform(-2.0, 2.0, (M, D))
    theta = np.concatenate([0.1 * np.arange(D) - 0.2, 0.3 * rng.standard_normal(D * lam), [0.2]])
    h = _capi.Handle(lib, 0)
    h.set_data(X[:N], Y[:N])
    h.set_kernel(_capi.KERNEL_SE_ARD, theta, NOISE)
    h.set_profiling(prof)
    assert h.compute() == 0

    def call(label, fn, names, times=None):
        res, launches = traced(lib, fn)
        report(np, name, label, launches, dict(zip(names, res)), times() if times and prof else None)

    call("query_batch", lambda: h.query_batch(Xq), ("kta", "var"))
    call("query_batch.kta", lambda: h.query_batch(Xq, want_var=False), ("kta", "var"))
    call("query_batch.var", lambda: h.query_batch(Xq, want_mu=False), ("kta", "var"))

    def cross():  # a caller-supplied cross kernel: N x M, column-major
        Ks = np.asfortranarray(np.exp(-0.5 * ((X[:N, None, :] - Xq[None, :, :]) ** 2).sum(axis=2)))
        kta, zz = np.zeros((M, P), order="F"), np.zeros(M)
        dp = lambda a: a.ctypes.data_as(_capi._dp)
        assert lib.fn("query_batch_cross")(h._h, dp(Ks), M, dp(kta), dp(zz)) == 0
        return kta, zz

    call("query_batch_cross", cross, ("kta", "zz"))
    grad_names = ("kta", "var", "dkta", "dvar")
    call("query_batch_grad", lambda: h.query_batch_grad(Xq), grad_names, h.query_grad_phase_ms)
    call("query_batch_grad.dkta", lambda: h.query_batch_grad(Xq, want=("dkta",)), grad_names, h.query_grad_phase_ms)
    call("joint_query", lambda: h.joint_query(Xq, 1e-6), ("kta", "cov"), h.joint_phase_ms)
    Z = rng.standard_normal((M, S, P))
    call("joint_draws", lambda: h.joint_draws(Xq, Z, 1e-6), ("status", "F", "argmax", "fmax"), h.joint_phase_ms)
    Om, ph = rng.standard_normal((R, D + lam)), rng.uniform(0.0, 2.0 * np.pi, R)
    W, E = rng.standard_normal((R, S, P)), rng.standard_normal((N, S, P))
    paths = []
    call("paths_create", lambda: paths.append(h.paths(R, S, Om, ph, W, E)) or (), (), lambda: paths[0].phase_ms())
    call("paths_eval", lambda: paths[0].eval(Xq), ("F", "dF"), lambda: paths[0].phase_ms())
    call("paths_argmax", lambda: paths[0].argmax(Xq), ("argmax", "fmax"), lambda: paths[0].phase_ms())
    paths[0].close()
    call("add_samples", lambda: (h.add_samples(X[N:], Y), h.get_alpha()), ("status", "alpha"))
    call("add_samples.query_batch", lambda: h.query_batch(Xq), ("kta", "var"))
    h.close()


def run_sparse_case(np, _capi, name):
    N, M, T, _, _ = SPARSE_CASES[name]
    lib = _capi.load_engine()
    X, Y = problem(np, N, 2, 4000)
    Xt = np.random.default_rng(4001).uniform(-2.0, 2.0, (T, D))
    for prof in (False, True):
        h = _capi.SparseHandle(lib, 0)
        h.set_data(X, Y)
        h.set_pseudo(X[:: N // M][:M])
        h.set_hparams(0.1 * np.arange(D) - 0.2, 0.1, np.log(NOISE), 1e-6)
        h.set_profiling(prof)
        tag = ".prof" if prof else ""
        st, launches = traced(lib, h.compute)
        report(np, name, "sp_compute" + tag, launches, {"status": st, "nlml": h.nlml(), "bet": h.get_bet(), "ep": h.get_ep(), "Lm": np.tril(h.get_Lm())},
               h.phase_ms() if prof else None)
        (mu, s2), launches = traced(lib, lambda: h.predict(Xt))
        report(np, name, "sp_predict" + tag, launches, {"mu": mu, "s2": s2}, h.phase_ms() if prof else None)
        (st, gx, gh), launches = traced(lib, h.grad)
        report(np, name, "sp_grad" + tag, launches, {"status": st, "d_xb": gx, "d_hp": gh}, h.grad_phase_ms() if prof else None)
        h.close()


def run_acq_case(np, _capi, name):
    N, M, prof, _, _ = ACQ_CASES[name]
    P, A, B, S, K = 4, 33, 20, 65, 65
    lib = _capi.load_engine()
    X, Y = problem(np, N, P, 6000)
    rng = np.random.default_rng(6001)
    Xc, Xa, Xb = (rng.uniform(-2.0, 2.0, (n, D)) for n in (M, A, B))
    h = _capi.Handle(lib, 0)
    h.set_data(X, Y)
    h.set_kernel(_capi.KERNEL_SE_ARD, 0.1 * np.arange(D + 1) - 0.2, NOISE)
    h.set_profiling(prof)
    assert h.compute() == 0

    def call(label, fn, names, times=None):
        res, launches = traced(lib, fn)
        report(np, name, label, launches, dict(zip(names, res)), times() if times and prof else None)

    add = 0.05 * rng.standard_normal((M, P))  # the caller's means, column j for belief j
    mu, sd = rng.standard_normal((M, P)), 0.1 + rng.random((M, P))  # host-supplied beliefs
    # the knowledge gradient
    names = ("status", "kg", "var", "cov")
    mu_a, mu_c = rng.standard_normal(A), rng.standard_normal(M)
    call("kg_batch", lambda: h.kg_batch(Xa, Xc, 0.1), names, h.kg_phase_ms)
    call("kg_batch.self", lambda: h.kg_batch(Xa, Xc, 0.1, with_self=True), names, h.kg_phase_ms)
    call("kg_batch.self.mu", lambda: h.kg_batch(Xa, Xc, 0.1, with_self=True, mu_a=mu_a, mu_c=mu_c), names, h.kg_phase_ms)
    call("kg_batch.mu.kg", lambda: h.kg_batch(Xa, Xc, 0.1, mu_a=mu_a, mu_c=mu_c, want=("kg",)), names, h.kg_phase_ms)
    call("kg_batch.self.var_cov", lambda: h.kg_batch(Xa, Xc, 0.1, with_self=True, want=("var", "cov")), names, h.kg_phase_ms)
    call("kg_envelope", lambda: h.kg_envelope(mu_a, rng.standard_normal((A, M)), ldb=A + 3), ("status", "kg", "nseg"))
    # the expected hypervolume improvement of outputs (2, 0)
    ref = (float(Y[:, 2].min()) - 0.1, float(Y[:, 0].min()) - 0.1)
    rc, F = _capi.ehvi2_front(Y[:, [2, 0]], ref)
    assert rc == 0 and len(F) >= 2
    names = ("status", "ehvi", "partials", "mu", "var")
    call("ehvi2_values", lambda: h.ehvi2_values(F, ref, mu[:, 0], sd[:, 0], mu[:, 1], sd[:, 1]), ("status", "ehvi", "partials"))
    call("ehvi2_values.ehvi", lambda: h.ehvi2_values(F, ref, mu[:, 0], sd[:, 0], mu[:, 1], sd[:, 1], want_partials=False), ("status", "ehvi", "partials"))
    call("ehvi2_batch.add", lambda: h.ehvi2_batch(Xc, F, ref, 2, 0, add[:, :2], 0.1), names, h.ehvi_phase_ms)
    call("ehvi2_batch", lambda: h.ehvi2_batch(Xc, F, ref, 2, 0), names, h.ehvi_phase_ms)
    call("ehvi2_batch.partials_var", lambda: h.ehvi2_batch(Xc, F, ref, 2, 0, add[:, :2], 0.1, want=("partials", "var")), names, h.ehvi_phase_ms)
    # constrained expected improvement: the objective output 1, constraints on outputs (3, 0, 2)
    thr = np.array([-0.3, 0.0, 0.2])
    names = ("status", "logcei", "terms", "partials", "mu", "var")
    for with_ei, C in ((1, 3), (1, 0), (0, 3)):
        tag = f".ei{with_ei}.c{C}"
        vals = lambda want: h.logcei_values(thr[:C], mu[:, 1:1 + C], sd[:, 1:1 + C], mu[:, 0], sd[:, 0], f_best=0.5, with_ei=with_ei, want=want)
        call("logcei_values" + tag, lambda: vals(("terms", "partials")), names[:4])
        call("logcei_values" + tag + ".partials", lambda: vals(("partials",)), names[:4])
    for with_ei, C in ((1, 3), (1, 0), (0, 3), (0, 0)):
        tag = f".ei{with_ei}.c{C}"
        fused = lambda mean_add, **kw: h.logcei_batch(Xc, thr[:C], [3, 0, 2][:C], out0=1, f_best=0.5, with_ei=with_ei, mean_add=mean_add, **kw)
        call("logcei_batch" + tag + ".add", lambda: fused(add[:, :1 + C], var_add=0.1), names, h.cei_phase_ms)
        call("logcei_batch" + tag, lambda: fused(None), names, h.cei_phase_ms)
        call("logcei_batch" + tag + ".terms_mu", lambda: fused(add[:, :1 + C], var_add=0.1, want=("terms", "mu")), names, h.cei_phase_ms)
    # max-value entropy search over outputs (2, 0)
    ystar = 1.0 + 0.3 * np.abs(rng.standard_normal((K, 2)))
    names = ("status", "logmes", "terms", "partials", "mu", "var")
    call("mes_values", lambda: h.mes_values(ystar, mu[:, :2], sd[:, :2]), names[:4])
    call("mes_values.terms", lambda: h.mes_values(ystar, mu[:, :2], sd[:, :2], want=("terms",)), names[:4])
    call("mes_batch.add", lambda: h.mes_batch(Xc, ystar, [2, 0], add[:, :2], 0.1), names, h.mes_phase_ms)
    call("mes_batch", lambda: h.mes_batch(Xc, ystar, [2, 0]), names, h.mes_phase_ms)
    call("mes_batch.partials_var", lambda: h.mes_batch(Xc, ystar, [2, 0], add[:, :2], 0.1, want=("partials", "var")), names, h.mes_phase_ms)
    # noisy expected improvement of output 1 over a baseline of B points
    Z, mean_b = rng.standard_normal((B, S)), 0.05 * rng.standard_normal(B)
    names = ("status", "lognei", "fplus", "mu", "var", "cvar", "cmean")
    call("lognei_values", lambda: h.lognei_values(rng.standard_normal(S), rng.standard_normal((S, M)), sd[:, 0]), ("status", "lognei", "terms"))
    call("lognei_values.lognei", lambda: h.lognei_values(rng.standard_normal(S), rng.standard_normal((S, M)), sd[:, 0], want=()), ("status", "lognei", "terms"))
    call("lognei_batch.add", lambda: h.lognei_batch(Xc, Xb, Z, 1, 1e-6, mean_b=mean_b, mean_add=add[:, 0]), names, h.nei_phase_ms)
    call("lognei_batch", lambda: h.lognei_batch(Xc, Xb, Z, 1, 1e-6), names, h.nei_phase_ms)
    call("lognei_batch.mu_cvar", lambda: h.lognei_batch(Xc, Xb, Z, 1, 1e-6, mean_b=mean_b, mean_add=add[:, 0], want=("mu", "cvar")), names, h.nei_phase_ms)
    h.close()


def run_shell_case(np, _capi, name):
    """The switches of the panel code are read by gpe_create: set between the creates, they differ from handle to handle."""
    lib = _capi.load_engine()
    theta = 0.1 * np.arange(D + 1) - 0.2
    panel_switches = ("GPE_TAIL_MAX", "GPE_PANEL256", "GPE_PANEL_HANDOVER")

    def call(label, fn, names):
        res, launches = traced(lib, fn)
        report(np, name, label, launches, dict(zip(names, res)))

    def evaluate(h):
        assert h.compute() == 0 and h.flow_retries() == 0 and h.handover_reruns() == 0
        return np.tril(h.get_L()), h.get_alpha(), np.float64(h.log_lik())

    def panels(tag, env, evaluations):
        for k in panel_switches:
            os.environ.pop(k, None)
        os.environ.update(env)
        h = _capi.Handle(lib, 0)
        h.set_data(*problem(np, 520, 1, 5000))
        h.set_kernel(_capi.KERNEL_SE_ARD, theta, NOISE)
        for i in range(evaluations):
            call(f"{tag}.compute{i}", lambda: evaluate(h), ("L", "alpha", "log_lik"))
        h.close()

    # 1. step-by-step panels without the hand-over: the head tiles of both halves are written and copied into the factor
    panels("stepped", {"GPE_TAIL_MAX": "0", "GPE_PANEL256": "0", "GPE_PANEL_HANDOVER": "0"}, 2)
    # 2. the pooled shell under the one-launch panels: both polled buffers, the flag tile of a block that has been used
    panels("panel256", {"GPE_TAIL_MAX": "0"}, 3)
    # 3. ... and under the small path, P = 2: from an empty model to n = 4, new observations, one point, five points
    del os.environ["GPE_TAIL_MAX"]
    X, Y = problem(np, 4, 2, 5001)
    Xq = np.random.default_rng(5002).uniform(-2.0, 2.0, (5, D))
    h = _capi.Handle(lib, 0)
    h.set_kernel(_capi.KERNEL_SE_ARD, theta, NOISE)
    for n in range(4):
        call(f"small.add_sample{n}", lambda: (h.add_sample(X[n], Y[: n + 1]), h.get_alpha(), np.float64(h.log_lik())), ("status", "alpha", "log_lik"))
    call("small.update_alpha", lambda: (h.update_alpha(0.5 - Y), h.get_alpha(), np.float64(h.log_lik())), ("status", "alpha", "log_lik"))
    call("small.query1", lambda: h.query_batch(Xq[:1]), ("kta", "var"))
    call("small.query5", lambda: h.query_batch(Xq), ("kta", "var"))
    # three add_samples, update_alpha and the two queries took the one-launch path: 6 (hashed below, in words on stderr)
    print(f"shell: {h.small_calls()} calls served by the small path", file=sys.stderr)
    report(np, name, "small.calls", [], {"small_calls": np.int64(h.small_calls())})
    h.close()


def run_case(name, root):
    sys.path.insert(0, str(root))
    import numpy as np

    from limbo_amd import _capi

    assert Path(_capi.__file__).resolve().is_relative_to(root), _capi.__file__
    if name == "lifecycle":
        return run_lifecycle(np, _capi)
    if name in QUERY_CASES:
        return run_query_case(np, _capi, name)
    if name in SPARSE_CASES:
        return run_sparse_case(np, _capi, name)
    if name in ACQ_CASES:
        return run_acq_case(np, _capi, name)
    if name in SHELL_CASES:
        return run_shell_case(np, _capi, name)
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
    _, launches = traced(lib, evaluate)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    out = {
        "case": name,
        "N": N,
        "P": P,
        "launches": launches,
        "L_sha256": [sha(np.tril(h.get_L())) for h in hs],
        "alpha_sha256": [sha(h.get_alpha()) for h in hs],
        "log_lik_bits": [struct.pack(">d", h.log_lik()).hex() for h in hs],
    }
    for h in hs:
        h.close()
    print(json.dumps(out), flush=True)


def compact(rec, kernels, seen):
    """A per-call line as it is printed: every launch as kernel index:grid[:block][@stream] (the grid without its trailing ones,
    the block unless it is 256, the stream index unless it is 0, `*n` behind a launch repeated n times in a row), the hashes cut to
    16 digits.  Nothing of the sequence is lost."""
    runs = []
    for s, k, grid, block in rec["launches"]:
        while len(grid) > 1 and grid[-1] == 1:
            grid = grid[:-1]
        e = f"{kernels.setdefault(k, len(kernels))}:{','.join(map(str, grid))}" + (f":{block}" if block != 256 else "") + (f"@{s}" if s else "")
        if runs and runs[-1][0] == e:
            runs[-1][1] += 1
        else:
            runs.append([e, 1])
    seq = " ".join(e if n == 1 else f"{e}*{n}" for e, n in runs)
    first = seen.setdefault(seq, f"{rec['case']}/{rec['call']}")  # a sequence printed before: "= the call that made it first"
    rec["launches"] = seq if first == f"{rec['case']}/{rec['call']}" else "= " + first
    rec["sha256"] = {k: v and v[:16] for k, v in rec["sha256"].items()}
    if "times_finite_nonneg" in rec:
        rec["times_finite_nonneg"] = all(rec["times_finite_nonneg"].values())
    return json.dumps(rec, separators=(",", ":"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent))
    ap.add_argument("--cases", default=",".join(ALL_CASES))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    root = Path(a.root).resolve()
    if a.child:
        run_case(a.child, root)
        return 0
    kernels = {}  # (the per-call lines name their kernels by index into this table, printed last)
    seen = {}
    status = 0
    for name in a.cases.split(","):
        env = {k: v for k, v in os.environ.items() if not k.startswith("GPE_")}
        env.update(ALL_CASES[name][-2])
        per_call = name not in CASES
        try:
            r = subprocess.run([sys.executable, __file__, "--root", str(root), "--child", name], env=env, timeout=CHILD_TIMEOUT_S,
                               stdout=subprocess.PIPE if per_call else None, text=True)
            rc = r.returncode
            for ln in (r.stdout or "").splitlines():
                print(compact(json.loads(ln), kernels, seen), flush=True)
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"case {name}: the child ended with status {rc}; stopping", file=sys.stderr)
            status = 1
            break
    if kernels:
        print(json.dumps({"kernels": list(kernels)}), flush=True)
    return status


if __name__ == "__main__":
    sys.exit(main())
