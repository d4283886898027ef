"""Builds tests/native/denoise_parts_check.cpp (the chunk plan and denoise_parts_error, no GPU) and asks
it a list of cases; shared by tests/test_denoise_parts_plan.py and tests/test_denoise_parts_params.py."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def build_checker(tmp_dir):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found")
    exe = str(tmp_dir / "denoise_parts_check")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe,
                           os.path.join(HERE, "native", "denoise_parts_check.cpp")])

    def ask(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        answers = out.stdout.splitlines()
        assert len(answers) == len(lines)
        return [a.split("|") for a in answers]
    return ask
