"""The device libm port (dmath.h: glibc 2.35 sinf/cosf algorithm in double precision) against
the host glibc the reference links (glm::sin / glm::cos -> sinf / cosf).  Host build of the
same source; the GPU builds of all five functions (sinf / cosf, acosf, atanf, atan2f, logf, and
logf through the volume kernel's LDS table) are checked in test_gpu_probe.py, on grids that hold
every boundary constant of the source.  An exhaustive sweep (stride 1) over [-120, 120], the whole
domain of glibc_sincosf, found 0 mismatches in 2.25e9 values; CI runs a strided sweep.  The sweeps
were repeated on the branch-free forms (glibc_sincosf, and acosf / atanf with one quotient
evaluation per lane): 0 mismatches."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found")
    exe = str(tmp_path_factory.mktemp("libm") / "libm_check")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-builtin", "-o", exe,
                           os.path.join(HERE, "native", "libm_port_check.cpp")])
    return exe


@pytest.mark.parametrize("stride,limit", [(97, "6.2831855"), (7919, "100.0")])
def test_sincos_port_matches_glibc(checker, stride, limit):
    out = subprocess.run([checker, str(stride), limit], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 mismatches" in out.stdout


# Windows at stride 1 around multiples of pi/2 (11, 37 and 74 of them), where the reduction x - n * pi/2
# cancels: the unfused form of that step differed from the host's FMA build of glibc there and only there
# (34 floats of the 2.2e9 in [-120, 120], found by test_gpu_probe.py's grid; fused: 0 mismatches, stride 1).
@pytest.mark.parametrize("start,limit", [("17.27", "17.29"), ("58.11", "58.13"), ("116.23", "116.25")])
def test_sincos_port_matches_glibc_where_the_reduction_cancels(checker, start, limit):
    out = subprocess.run([checker, "1", limit, start], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 mismatches" in out.stdout


@pytest.fixture(scope="module")
def inv_checker(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("libm_inv") / "libm_inv_check")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-builtin", "-o", exe,
                           os.path.join(HERE, "native", "libm_inv_check.cpp")])
    return exe


# Exhaustive runs (stride 1) in this container: acosf 2.13e9 values over [-1, 1] (+ beyond),
# atanf all 4.28e9 non-NaN-payload patterns, atan2f 3e8 random pairs: 0 mismatches.
# logf (FMA form): all 2.14e9 positive patterns, 0 mismatches.
@pytest.mark.parametrize("args", [("acos", "101"), ("atan", "1009"), ("atan2", "3000000", "5"), ("log", "211")])
def test_inverse_trig_ports_match_glibc(inv_checker, args):
    """glibc 2.35 acosf / atanf / atan2f / logf restated in dmath.h (environment light mapping,
    UniformSampleSphere, SampleExponentialDecay)."""
    out = subprocess.run([inv_checker, *args], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 mismatches" in out.stdout
