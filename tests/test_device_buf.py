"""Who frees device memory and events (csrc/host/device_buf.h), checked on the CPU.

tests/native/device_buf_check.cpp runs the header over a counting fake backend: one scripted sequence
of reserves (growing, equal, smaller, zero, on two device ordinals, a group of three buffers with one
capacity), a move, a release and a scope exit, once without a failure and once for every N with the
N-th allocation failing.  In every run it checks that a failed reserve leaves the buffer null with
capacity 0 and that the very next reserve of it allocates and succeeds; that no block is freed twice
or looked at after it was freed; that a buffer never has two live blocks (the old one is freed before
the new one is allocated, and a group frees all of its buffers before it allocates any); that every
free happens with the owning device current and the caller's current device is what it was after
every call; that a smaller or equal reserve makes no backend call; and that no block and no event is
live at the end."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
RUN = re.compile(r"run (\d+) allocs (\d+) hit (\d+) checks (\d+) (ok|FAIL)$")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found")
    exe = str(tmp_path_factory.mktemp("device_buf") / "device_buf_check")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "native", "device_buf_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    lines = out.stdout.splitlines()
    broken = [line for line in lines if not RUN.match(line)]
    assert out.returncode == 0 and not broken, "\n".join(broken or lines[-5:]) + out.stderr
    return [tuple(int(v) for v in RUN.match(line).groups()[:4]) + (RUN.match(line).group(5),) for line in lines]


def test_every_failing_allocation_is_run(runs):
    """One run without a failure, then one per allocation of the sequence: none skipped."""
    n, length, hit, checks, verdict = runs[0]
    assert (n, hit, verdict) == (0, 0, "ok") and length >= 20 and checks > 0
    assert [r[0] for r in runs] == list(range(length + 1))


def test_every_run_holds(runs):
    length = runs[0][1]
    for n, allocs, hit, checks, verdict in runs[1:]:
        assert verdict == "ok", n
        assert hit == 1, n                      # the N-th allocation did fail
        assert allocs > length, n               # and the reserve after it allocated again
        assert checks >= runs[0][3], n          # nothing was cut short by the failure
