"""Where a drop-in model::GP lives (include/limbo_amd/limbo/model/gp/residency.hpp) on its own, under AddressSanitizer and UBSan.

limbo_amd::Residency is a plain value: no Eigen, no engine.  tests/cpp/test_residency.cpp applies every transition to every state
that any sequence of transitions reaches and compares every query with the table of DESIGN.md ("Residency"); it checks what a copy
starts with, and that the shadow of a host model stops being current with any host factor or alpha change and with another
hyper-parameter vector or noise."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_every_transition_from_every_reachable_state_follows_the_table():
    subprocess.check_call(["make", "-s", "-C", str(ROOT / "tests" / "cpp"), "test_residency"])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(ROOT / "tests" / "cpp" / "test_residency")], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
    assert "residency ok" in r.stdout
