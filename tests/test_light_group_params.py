"""The rules of a light-group call's arguments (csrc/host/stage_params.h light_groups_error,
light_mix_error), checked on the CPU: every message, in the order the rules are tested, and what passes."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
M_G = "n_groups must be 1..8"
M_NULL = "the light-group map is required"
M_LEN = "the light-group map must have one entry per light of the scene"
M_VALUE = "a light's group must be < n_groups"
M_PTRS = "the gains, the group images and the mixed image are required"
M_FINITE = "light-mix gains must be finite"


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found")
    exe = str(tmp_path_factory.mktemp("light_group_params") / "light_group_params_check")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "native", "light_group_params_check.cpp")])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        answers = out.stdout.splitlines()
        assert len(answers) == len(lines)
        return answers
    return run


def _groups(G, n, scene, null=0, values=()):
    return "groups %d %d %d %d " % (G, n, scene, null) + " ".join(map(str, values))


def test_light_groups_error(ask):
    cases = [
        (_groups(0, 2, 2, values=(0, 0)), M_G), (_groups(9, 2, 2, values=(0, 1)), M_G),
        (_groups(0, 2, 2, null=1), M_G),                      # the group count is tested first
        (_groups(2, 2, 2, null=1), M_NULL),
        (_groups(2, 1, 2, values=(0,)), M_LEN), (_groups(2, 3, 2, values=(0, 1, 1)), M_LEN),
        (_groups(2, 0, 2), M_LEN),
        (_groups(2, 2, 2, values=(0, 2)), M_VALUE), (_groups(1, 4, 4, values=(0, 0, 1, 0)), M_VALUE),
        (_groups(8, 2, 2, values=(8, 0)), M_VALUE), (_groups(2, 2, 2, values=(0, 4294967295)), M_VALUE),
        (_groups(2, 2, 2, values=(0, 1)), "ok"), (_groups(1, 2, 2, values=(0, 0)), "ok"),
        (_groups(8, 4, 4, values=(7, 0, 3, 7)), "ok"),
        (_groups(3, 2, 2, values=(0, 2)), "ok"),              # a group may hold no light
        (_groups(1, 0, 0), "ok"),                             # (a scene without lights is check_params's to refuse)
    ]
    got = ask([c for c, _w in cases])
    for (c, want), g in zip(cases, got):
        assert g == want, c


def test_light_mix_error(ask):
    one = "1 0.5 -0"
    cases = [
        ("mix 0 0 " + one, M_G), ("mix 9 0 " + " ".join(["1"] * 27), M_G), ("mix 0 7", M_G),
        ("mix 1 1 " + one, M_PTRS), ("mix 1 2 " + one, M_PTRS), ("mix 1 4 " + one, M_PTRS), ("mix 2 7", M_PTRS),
        ("mix 1 0 1 nan 1", M_FINITE), ("mix 1 0 inf 1 1", M_FINITE), ("mix 2 0 1 1 1 1 1 -inf", M_FINITE),
        ("mix 1 0 " + one, "ok"), ("mix 2 0 0 0 0 -1 2 3e38", "ok"),
        ("mix 1 0 1 1 1 nan", "ok"),                           # beyond 3 G gains nothing is read
        ("mix 8 0 " + " ".join(["0.25"] * 24), "ok"),
    ]
    got = ask([c for c, _w in cases])
    for (c, want), g in zip(cases, got):
        assert g == want, c
