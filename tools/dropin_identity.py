#!/usr/bin/env python3
"""Same headers, same bits: what the C++ drop-in's drivers print, per include tree.  The drivers of tests/cpp print every value with
%.17g, so a change of include/limbo_amd that is a refactor leaves the sha256 of every driver's output as it was.  Run it on two
include trees against the ONE libgpengine.so of this checkout and diff the outputs:

    git archive <parent> include | tar -x -C /tmp/parent
    python tools/dropin_identity.py /tmp/parent/include --cases host > parent.txt
    python tools/dropin_identity.py include --cases host > branch.txt

INCLUDE is a directory that holds gpe.h and limbo_amd/.  The drivers are compiled against it with the flags of tests/cpp/Makefile
into --bin (default: a temporary directory; --no-build: take the programs that are there, built where there is a compiler to spare).
Every driver's input is written by the test modules' own run_driver from their own problem generators (dropin_problem, with_steps
and their siblings in tests/test_*_host.py): inside those modules `subprocess` is replaced by a recorder that runs the program
built here in place of the test's, under its own time limit.  One line per case: name, exit status, sha256 of stdout.  The first
case that does not end with status 0, or whose model did not live where the case wants it (the host_resident lines of the drivers
that print them: all 1 or all 0, or the per-step sequence of the residency walk), ends the run.  --sanitize builds with -fsanitize=address,undefined as `make -C tests/cpp asan` does (other bits: the statuses count, not
the hashes): stand-alone programs on the host cases, on a machine's CPU only.

--cases host: below Params::gpu::min_n_for_gpu with the host tests' HOST_ENV, nothing touches the device.  --cases device: n = 300
with LIMBO_AMD_MIN_N_FOR_GPU=0, the size of the device drop-in tests.

--ab OTHER_BIN (with --cases device): after the list, the wall time of the whole process of the CEI and MES device cases, the programs
of OTHER_BIN and of --bin interleaved, --runs each; medians and spreads on stdout behind the case lines.
"""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DRIVERS = ("test_cei_dropin", "test_mes_dropin", "test_ehvi_dropin", "test_nei_dropin", "test_kg_dropin", "test_batch_select_dropin",
           "test_query_grad_host", "test_query_grad_dropin", "test_host_path", "test_add_samples", "test_remove_samples", "test_residency_walk")
DEVICE_ENV = {"LIMBO_AMD_MIN_N_FOR_GPU": "0"}
RUN_LIMIT_S = 120
AB_CASES = ("cei.c2.obs1.steps", "mes.p2.obs1.steps")


SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g", "-O1"]  # tests/cpp/Makefile's


def build(include, bindir, sanitize):
    cxx = os.environ.get("CXX", "g++")
    for d in DRIVERS:
        subprocess.check_call([cxx, "-std=c++17"] + (SAN if sanitize else ["-O2"]) + ["-Wall", "-Wno-unused-variable", f"-I{include}/limbo_amd", f"-I{ROOT}/oracle/ref_build/shim",
                               "-o", str(bindir / d), str(ROOT / "tests" / "cpp" / (d + ".cpp")), f"-L{ROOT}/limbo_amd", "-lgpengine",
                               "-Wl,-rpath,/opt/rocm/lib", "-lpthread"])


class Recorder:
    """`subprocess` as a test module sees it: run() starts the program of the same name from `bindir` under its own time limit and
    keeps what it did"""
    PIPE = subprocess.PIPE

    def __init__(self, bindir):
        self.bindir = bindir
        self.last = None

    def command(self, argv, bindir=None):
        return ["timeout", "-k", "10", str(RUN_LIMIT_S), str((bindir or self.bindir) / Path(argv[0]).name)] + [str(a) for a in argv[1:]]

    def environment(self, kw):
        env = dict(kw.get("env") or os.environ)
        env["LD_LIBRARY_PATH"] = str(ROOT / "limbo_amd") + os.pathsep + env.get("LD_LIBRARY_PATH", "")
        env.setdefault("ASAN_OPTIONS", "detect_leaks=0:halt_on_error=1")  # (read by a --sanitize build alone)
        env.setdefault("UBSAN_OPTIONS", "halt_on_error=1:print_stacktrace=1")
        return env

    @staticmethod
    def check_call(*a, **kw):  # (a test module's `make`: the programs are built here)
        return 0

    def run(self, argv, **kw):
        self.last = (argv, kw)
        self.result = subprocess.run(self.command(argv), capture_output=True, text=True, env=self.environment(kw))
        return self.result

    def wall_time(self, bindir):
        argv, kw = self.last
        t0 = time.perf_counter()
        r = subprocess.run(self.command(argv, bindir), capture_output=True, text=True, env=self.environment(kw))
        return time.perf_counter() - t0, r.returncode


# host_resident after every step of tests/cpp/test_residency_walk (tests/test_residency_walk.py, tests/test_gpu_residency_walk.py).  A
# model pinned to the device by compute_inv_kernel() stays pinned when it is emptied, so the refill of `cross` stays on the device.
WALK = {"host": "1 1 1 1 1 1 1 1 1 0 1", "cross": "1 1 0 1 1 1 1 0 0 0 0 0 0", "device": "0 0 0 0 0 0 0 0 0 0 0 0 0"}


def cases(path, rec):
    """(name, module, call[, host_resident lines expected]): call(run_driver, tmp_path) writes the input and runs the driver"""
    import numpy as np

    from tests import test_batch_select as BS
    from tests import test_cei_host as CEI
    from tests import test_ehvi_host as EHVI
    from tests import test_kg_host as KG
    from tests import test_mes_host as MES
    from tests import test_nei_host as NEI
    from tests import test_query_grad_host as QG
    from tests.sparse_ref import ELL6 as LENGTHS6

    host = path == "host"
    env = CEI.HOST_ENV if host else DEVICE_ENV
    n, M = (40, 12) if host else (300, 16)
    D, hp, nid = (3, None, 0) if host else (6, np.log(list(LENGTHS6) + [1.0]), 1)  # (the length scales and the noise of the device tests)
    out = []

    def cei(name, C, observation, steps=True, with_ei=1, search=0):
        X, Y, thr, Q = CEI.dropin_problem(D, n, C, M, 77 + C)
        Q = np.clip(Q, 0.0, 1.0) if not host else Q
        out.append((f"cei.{name}", CEI, lambda run, tmp: run(tmp, 0, 0, X, Y, thr, CEI.with_steps(Q) if steps else Q, noise_id=nid, observation=observation,
                                                          hp=hp, with_ei=with_ei, search=search, env=env)))

    cei("c1.obs0.steps", 1, 0)
    cei("c2.obs1.steps", 2, 1)
    cei("c3.obs0.no_ei", 3, 0, steps=False, with_ei=0)
    cei("c0.obs1.steps", 0, 1)
    cei("c2.obs1.search", 2, 1, steps=False, search=1)

    def mes(name, P, K, observation, search=0):
        X, Y, Q = MES.dropin_problem(D, n, P, M, 77 + P)
        Q = np.clip(Q, 0.0, 1.0) if not host else Q
        out.append((f"mes.{name}", MES, lambda run, tmp: run(tmp, 0, 0, X, Y, Q[:2] if search else MES.with_steps(Q), K, 11, noise_id=nid,
                                                          observation=observation, hp=hp, search=search, env=env)))

    mes("p1.obs0.steps", 1, 8, 0)
    mes("p2.obs1.steps", 2, 8, 1)
    mes("p3.obs0.steps", 3, 16, 0)
    mes("p1.obs1.search", 1, 8, 1, search=1)

    for observation in (0, 1):
        X, Y, ref, Q = EHVI.dropin_problem(0, n, M, 60 + observation)
        out.append((f"ehvi.obs{observation}.steps", EHVI, lambda run, tmp, a=(X, Y, ref, Q, observation): run(
            tmp, 0, 0, a[0], a[1], a[1], a[2], EHVI.with_steps(a[3]), noise_id=observation, observation=a[4], env=env)))

    X, Y, Q, Xb, nhp = NEI.dropin_problem(n, M, 9, 21)
    out.append(("nei", NEI, lambda run, tmp: run(tmp, X, Y, Q, Xb, 7, 5, nhp, env=env)))

    for P, agg, with_self in ((1, 0, 1), (2, 1, 0)):
        Xk, Yk, Qa, Qc = KG.dropin_problem(0, P, n, 24, M, 10 * P + n)
        out.append((f"kg.p{P}.self{with_self}", KG, lambda run, tmp, a=(Xk, Yk, Qa, Qc, agg, with_self): run(tmp, 0, 0, *a, env=env)))

    for P, agg in ((1, 0), (2, 1)):
        Xs, Ys, Qs = BS.dropin_problem(0, P, n, M, 10 * P + n)
        out.append((f"batch_select.p{P}", BS, lambda run, tmp, a=(Xs, Ys, Qs, 8, agg): run(tmp, 0, 0, *a, env=env)))

    drv = "test_query_grad_host" if host else "test_query_grad_dropin"
    qenv = dict(QG.HOST_ENV) if host else DEVICE_ENV
    for kind in (QG.O.SE_ARD, QG.O.MATERN52):
        case = QG.dropin_problem(kind, n, 3, 2 if kind == QG.O.SE_ARD else 1, M, 40 + kind)
        out.append((f"query_grad.kind{kind}", QG, lambda run, tmp, c=case: run(drv, "grad", QG.grad_case_text(*c), tmp, qenv)))
    out.append(("query_grad.search", QG, lambda run, tmp: run(drv, "search", QG.search_case_text(n=n), tmp, qenv)))

    # the factor's life: compute / add_sample / add_samples / remove_samples and the walk across the host / device boundaries
    from tests import test_add_samples_host as AS
    from tests import test_host_path as HP

    none = []  # (these drivers print no host_resident line)
    if host:
        for kind, mean, P, Dh, n0, n1 in HP.CASES:  # the problems of test_host_path_vs_reference_and_oracle
            rng = np.random.default_rng(100 * kind + 10 * mean + P)
            Xh = rng.uniform(-1, 1, size=(n1, Dh))
            Yh = np.stack([np.cos((p + 1.5) * Xh.sum(axis=1)) + 0.3 * Xh[:, 0] for p in range(P)], axis=1) + 0.05 * rng.normal(size=(n1, P))
            Qh = np.concatenate([rng.uniform(-1, 1, size=(4, Dh)), Xh[:2]])
            out.append((f"host_path.k{kind}.m{mean}.p{P}", HP, lambda run, tmp, a=(kind, mean, Xh, Yh, n0, Qh): HP._run(tmp, *a), none))
        out.append(("host_path.arguments", HP, lambda run, tmp: HP.test_acquisition_arguments_on_the_host(), none))
    for kind, mean, P, Da, n0, n1 in (AS.CASES if host else [(0, 0, 1, 6, 300, 340)]):
        Xa, Ya, Qa = AS.problem(kind, mean, P, Da, n1)

        def add(run, tmp, a=(kind, mean, Xa, Ya, n0, Qa)):
            AS.write_input(tmp / "in.txt", *a)
            rec.run(["test_add_samples", tmp / "in.txt"] + ([] if host else ["device"]))

        out.append((f"add_samples.k{kind}.m{mean}.p{P}", AS, add, none))
    out.append(("remove_samples", AS, lambda run, tmp: rec.run(["test_remove_samples"] + ([] if host else ["device"])), none))
    for mode in (["host"] if host else ["cross", "device"]):
        out.append((f"walk.{mode}", AS, lambda run, tmp, m=mode: rec.run(["test_residency_walk", m]), WALK[mode].split()))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("include", help="the include tree the drivers are compiled against (holds gpe.h and limbo_amd/)")
    ap.add_argument("--cases", choices=("host", "device"), default="host")
    ap.add_argument("--bin", help="where the drivers are built and run from (default: a temporary directory)")
    ap.add_argument("--no-build", action="store_true", help="run the programs --bin already holds")
    ap.add_argument("--sanitize", action="store_true", help="build with -fsanitize=address,undefined (host cases, stand-alone programs)")
    ap.add_argument("--ab", help="the --bin of another include tree: time the CEI and MES device cases against it")
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as scratch:
        bindir = Path(a.bin).resolve() if a.bin else Path(scratch) / "bin"
        bindir.mkdir(parents=True, exist_ok=True)
        if not a.no_build:
            build(Path(a.include).resolve(), bindir, a.sanitize)
        rec = Recorder(bindir)
        timings = []
        for name, mod, call, *expect in cases(a.cases, rec):
            mod.subprocess = rec
            if hasattr(mod, "DRIVER"):
                mod.build_driver = lambda d=mod.DRIVER: d  # (the recorder takes the program of that name from bindir)
            tmp = Path(scratch) / name
            tmp.mkdir()
            try:
                call(getattr(mod, "run_driver", None), tmp)
            except AssertionError:
                pass  # (run_driver's own check of the status: the line below says it)
            r = rec.result
            print(f"{a.cases}/{name}", r.returncode, hashlib.sha256(r.stdout.encode()).hexdigest(), flush=True)
            # the path the case is about was the one taken: the drivers say where the model lived
            where = [w for ln in r.stdout.splitlines() if ln.startswith("host_resident") for w in ln.split()[1:]]
            lived = where == expect[0] if expect else bool(where) and set(where) == {"1" if a.cases == "host" else "0"}
            if r.returncode != 0 or not lived or "runtime error" in r.stderr:
                print(f"case {name}: status {r.returncode}, host_resident {where}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
                return 1
            if a.ab and name in AB_CASES:
                t = {"other": [], "this": []}
                for _ in range(a.runs):
                    for side, d in (("other", Path(a.ab).resolve()), ("this", bindir)):
                        dt, rc = rec.wall_time(d)
                        if rc != 0:
                            print(f"timing {name} ({side}): status {rc}; stopping", file=sys.stderr)
                            return 1
                        t[side].append(dt)
                timings.append((name, t))
        for name, t in timings:
            for side in ("other", "this"):
                v = sorted(t[side])
                print(f"# wall time {name} {side}: median {statistics.median(v):.3f} s, min {v[0]:.3f} s, max {v[-1]:.3f} s, runs {len(v)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
