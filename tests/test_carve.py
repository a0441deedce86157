"""The typed scratch carver of the query family (limbo_amd/csrc/carve.h) on the host, under AddressSanitizer and UBSan.

Every query-side call declares its regions of gpe_ctx::dQuery once (QueryScratch::carve, query.hpp); a region left out of the
count, or one that starts unaligned, would be an out-of-bounds device write no CPU test sees.  The carver itself needs no GPU:
tests/cpp/test_carve.cpp lays out mixed-type regions in a malloc of exactly the counted size and writes all of them."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_carver_regions_are_aligned_disjoint_and_inside_the_counted_size():
    subprocess.check_call(["make", "-s", "-C", str(ROOT / "tests" / "cpp"), "test_carve"])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(ROOT / "tests" / "cpp" / "test_carve")], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
    assert "carve ok" in r.stdout
