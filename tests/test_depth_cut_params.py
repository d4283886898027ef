"""The rules of a depth-cut call's arguments (csrc/host/stage_params.h depth_cuts_error), checked on the
CPU: every message, in the order the rules are tested, and what passes."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
M_K = "n_cuts must be 1..8"
M_NULL = "the depth cuts are required"
M_ZERO = "a depth cut must be at least 1"
M_ABOVE = "a depth cut must not exceed the bounce limit"
M_ORDER = "depth cuts must be strictly ascending"


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found")
    exe = str(tmp_path_factory.mktemp("depth_cut_params") / "depth_cut_params_check")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "native", "depth_cut_params_check.cpp")])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        answers = out.stdout.splitlines()
        assert len(answers) == len(lines)
        return answers
    return run


def _cuts(K, bounces, values=(), null=0):
    return "cuts %d %d %d " % (K, bounces, null) + " ".join(map(str, values))


def test_depth_cuts_error(ask):
    cases = [
        (_cuts(0, 12), M_K), (_cuts(9, 12, range(1, 10)), M_K),
        (_cuts(0, 12, null=1), M_K),                           # the count is tested first
        (_cuts(2, 12, null=1), M_NULL),
        (_cuts(1, 12, (0,)), M_ZERO), (_cuts(3, 12, (0, 1, 2)), M_ZERO),
        (_cuts(1, 12, (13,)), M_ABOVE), (_cuts(3, 5, (1, 2, 6)), M_ABOVE), (_cuts(1, 12, (4294967295,)), M_ABOVE),
        (_cuts(1, 0, (1,)), M_ABOVE),                          # no cut fits a bounce limit of 0
        (_cuts(2, 12, (2, 2)), M_ORDER), (_cuts(3, 12, (1, 3, 2)), M_ORDER), (_cuts(2, 12, (5, 1)), M_ORDER),
        (_cuts(3, 12, (1, 2, 0)), M_ZERO),                     # per cut: its range before its order
        (_cuts(1, 12, (1,)), "ok"), (_cuts(1, 12, (12,)), "ok"), (_cuts(3, 12, (1, 2, 5)), "ok"),
        (_cuts(8, 12, range(1, 9)), "ok"), (_cuts(4, 16, (1, 3, 5, 16)), "ok"), (_cuts(8, 32, range(4, 33, 4)), "ok"),
    ]
    got = ask([c for c, _w in cases])
    for (c, want), g in zip(cases, got):
        assert g == want, c
