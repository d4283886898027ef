"""Depth cuts in the frame plan (csrc/host/frame_plan.h plan_frame), checked on the CPU: the new output
kind comes last and has no pass of its own (the cut records are the path kernel's, like the beauty's and
the light groups'), the new rules refuse with their own code and message after every earlier rule, a
request without cuts gets exactly the plan it got before (tests/test_frame_plan_lights.py's restatement
over its whole case grid), and a request with K cuts gets the beauty, then the cuts in order, and 16 K
bytes of record memory per sample."""
import os
import shutil
import subprocess

import pytest

import test_frame_plan as base
import test_frame_plan_lights as lights

HERE = os.path.dirname(os.path.abspath(__file__))
E_INVALID, E_UNSUPPORTED = base.E_INVALID, base.E_UNSUPPORTED
PATH, VOLUME = base.PATH, base.VOLUME
DEPTH_CUT = 9
M_MANY = "at most 8 depth cuts are supported"
M_BEAUTY = "depth cuts need the path kernel (the beauty)"
M_VOLUME = "depth cuts need the path integrator: the volume integrator has no depth-cut build"
M_ADAPTIVE = "depth cuts need a uniform render: not adaptive sampling"
M_ALONE = ("depth cuts are not rendered with the cascade, the mattes, AOVs, guides, the moment image or light groups in "
           "one call")


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found")
    return hipcc


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("frame_plan_depth") / "frame_plan_depth_check")
    subprocess.check_call([_hipcc(), "-O2", "-std=c++17", "-o", path, os.path.join(HERE, "native", "frame_plan_depth_check.cpp")])
    return path


@pytest.fixture(scope="module")
def checker(exe):
    def ask(cases, rules="frame"):
        lines = [rules + " %d %d %d %d %d %d %d %d %d %d %d %d" % c for c in cases]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        answers = out.stdout.splitlines()
        assert len(answers) == len(lines)
        return [base._parse(a) for a in answers]
    return ask


def restate(beauty, bits, moment, adaptive, K, matte, n_ids, integrator, gbits, max_follow, G, cuts):
    """A whole frame's plan with `cuts` depth cuts: the earlier rules first, then the cuts' own in their
    order, each with its message; else the beauty and the cuts ascending, no pass, 16 bytes per cut."""
    plan = lights.restate(beauty, bits, moment, adaptive, K, matte, n_ids, integrator, gbits, max_follow, G)
    if plan["code"] or not cuts:
        return plan
    if cuts > 8:
        return base._error(E_INVALID, M_MANY)
    if not beauty:
        return base._error(E_INVALID, M_BEAUTY)
    if integrator == VOLUME:
        return base._error(E_UNSUPPORTED, M_VOLUME)
    if adaptive:
        return base._error(E_UNSUPPORTED, M_ADAPTIVE)
    if K or matte or bits or gbits or moment or G:
        return base._error(E_UNSUPPORTED, M_ALONE)
    plan["outputs"] += [(DEPTH_CUT, j) for j in range(cuts)]
    plan["extra"] = 16 * cuts
    return plan


# the light groups' grid, without groups and with two
GRID = [c + (G,) for c in lights.GRID for G in (0, 2)]


def test_new_kind_comes_last_and_has_no_pass(exe):
    out = subprocess.run([exe, "constants"], capture_output=True, text=True, check=True).stdout.split()
    light_group, depth_cut, its_pass, n_passes, max_outputs, n_pass_of, max_cuts = map(int, out)
    assert depth_cut == light_group + 1 == lights.LIGHT_GROUP + 1 == DEPTH_CUT
    assert its_pass == n_passes  # the path kernel's own records: no PassKind added
    assert n_pass_of == 8 and max_cuts == 8 and max_outputs >= 1 + max_cuts


def test_without_cuts_the_plan_is_the_earlier_one(checker, tmp_path):
    """No cuts over the light groups' grid: the earlier restatement for a frame, and under both rule sets
    the answers of the earlier checker (tests/native/frame_plan_lights_check.cpp), which knows no cuts."""
    earlier = str(tmp_path / "frame_plan_lights_check")
    subprocess.check_call([_hipcc(), "-O2", "-std=c++17", "-o", earlier, os.path.join(HERE, "native", "frame_plan_lights_check.cpp")])
    for rules in ("frame", "buckets"):
        got = checker([c + (0,) for c in GRID], rules)
        lines = [rules + " %d %d %d %d %d %d %d %d %d %d %d" % c for c in GRID]
        out = subprocess.run([earlier], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        assert got == [base._parse(a) for a in out.stdout.splitlines()]
        if rules == "frame":
            for c, g in zip(GRID, got):
                assert g == lights.restate(*c), c


def test_cuts_match_the_rules(checker):
    cases = [c + (n,) for c in GRID for n in (1, 3, 8, 9)]
    seen = set()
    for c, got in zip(cases, checker(cases)):
        want = restate(*c)
        assert got == want, (c, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
        if got["code"] == 0:
            n = c[-1]
            assert got["outputs"] == [(base.BEAUTY, 0)] + [(DEPTH_CUT, j) for j in range(n)]  # beauty, then the cuts
            assert got["passes"] == [] and got["path"] == 1 and got["extra"] == 16 * n
        seen.add(got["message"])
    for m in (M_MANY, M_BEAUTY, M_VOLUME, M_ADAPTIVE, M_ALONE, ""):
        assert m in seen, m


def test_each_new_rule_alone(checker):
    many, nobeauty, volume, adaptive, cascade, mattes, aovs, gd, moment, groups, ok = checker([
        (1, 0, 0, 0, 0, 0, 0, PATH, 0, 0, 0, 9), (0, 0, 0, 0, 0, 0, 0, PATH, 0, 0, 0, 2), (1, 0, 0, 0, 0, 0, 0, VOLUME, 0, 0, 0, 2),
        (1, 0, 0, 1, 0, 0, 0, PATH, 0, 0, 0, 2), (1, 0, 0, 0, 2, 0, 0, PATH, 0, 0, 0, 2), (1, 0, 0, 0, 0, 1, 4, PATH, 0, 0, 0, 2),
        (1, 1, 0, 0, 0, 0, 0, PATH, 0, 0, 0, 2), (1, 0, 0, 0, 0, 0, 0, PATH, 3, 8, 0, 2), (1, 0, 1, 0, 0, 0, 0, PATH, 0, 0, 0, 2),
        (1, 0, 0, 0, 0, 0, 0, PATH, 0, 0, 2, 2), (1, 0, 0, 0, 0, 0, 0, PATH, 0, 0, 0, 8)])
    assert many == base._error(E_INVALID, M_MANY)
    assert nobeauty == base._error(E_INVALID, M_BEAUTY)
    assert volume == base._error(E_UNSUPPORTED, M_VOLUME)
    assert adaptive == base._error(E_UNSUPPORTED, M_ADAPTIVE)
    alone = base._error(E_UNSUPPORTED, M_ALONE)
    assert cascade == alone and mattes == alone and aovs == alone and gd == alone and moment == alone and groups == alone
    assert ok["code"] == 0 and len(ok["outputs"]) == 9 and ok["extra"] == 128


def test_bucket_rules_take_cuts_too(checker):
    (got,) = checker([(1, 0, 0, 0, 0, 0, 0, PATH, 0, 0, 0, 3)], rules="buckets")
    assert got["outputs"] == [(base.BEAUTY, 0), (DEPTH_CUT, 0), (DEPTH_CUT, 1), (DEPTH_CUT, 2)] and got["extra"] == 48
