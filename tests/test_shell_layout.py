"""The layout of a handle's shell (limbo_amd/csrc/shell_layout.h) on the host, under AddressSanitizer and UBSan.

The device block and the pinned block of a handle are carved by one header: the head tiles of either panel form, k_panel256's
polled buffers, the hand-over flag words, the log-likelihood partials, the small path's staging.  A region that reached into
its neighbour, or past its block, would be an out-of-bounds device write no CPU test sees.  The header needs no GPU:
tests/cpp/test_shell_layout.cpp pins every offset to its value, writes every region at its largest extent in host buffers of
exactly the block sizes and reads the patterns back."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_shell_regions_keep_their_offsets_are_disjoint_and_inside_their_blocks():
    subprocess.check_call(["make", "-s", "-C", str(ROOT / "tests" / "cpp"), "test_shell_layout"])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(ROOT / "tests" / "cpp" / "test_shell_layout")], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
    assert "shell layout ok: 2170880 + 18560 bytes" in r.stdout
