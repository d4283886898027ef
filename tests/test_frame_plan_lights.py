"""Light groups in the frame plan (csrc/host/frame_plan.h plan_frame), checked on the CPU: the new
output kind comes last and has no pass of its own (the group records are the path kernel's, like the
beauty's), the new rules refuse with their own code and message after every earlier rule, a request
without groups gets exactly the plan it got before (tests/test_frame_plan_guides.py's restatement over
its whole case grid), and a request with G groups gets the beauty, then the groups in order, and
16 G bytes of record memory per sample."""
import os
import shutil
import subprocess

import pytest

import test_frame_plan as base
import test_frame_plan_guides as guides

HERE = os.path.dirname(os.path.abspath(__file__))
E_INVALID, E_UNSUPPORTED = base.E_INVALID, base.E_UNSUPPORTED
PATH, VOLUME = base.PATH, base.VOLUME
LIGHT_GROUP = 8
M_MANY = "at most 8 light groups are supported"
M_BEAUTY = "light groups need the path kernel (the beauty)"
M_VOLUME = "light groups need the path integrator: the volume integrator has no light-group build"
M_ADAPTIVE = "light groups need a uniform render: not adaptive sampling"
M_ALONE = "light groups are not rendered with the cascade, the mattes, AOVs, guides or the moment image in one call"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found")
    path = str(tmp_path_factory.mktemp("frame_plan_lights") / "frame_plan_lights_check")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-o", path,
                           os.path.join(HERE, "native", "frame_plan_lights_check.cpp")])
    return path


@pytest.fixture(scope="module")
def checker(exe):
    def ask(cases, rules="frame"):
        lines = [rules + " %d %d %d %d %d %d %d %d %d %d %d" % c for c in cases]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        answers = out.stdout.splitlines()
        assert len(answers) == len(lines)
        return [base._parse(a) for a in answers]
    return ask


def restate(beauty, bits, moment, adaptive, K, matte, n_ids, integrator, gbits, max_follow, G):
    """A whole frame's plan with G light groups: the earlier rules first, then the groups' own in their
    order, each with its message; else the beauty and the groups ascending, no pass, 16 G bytes."""
    plan = guides.restate(beauty, bits, moment, adaptive, K, matte, n_ids, integrator, gbits, max_follow)
    if plan["code"] or not G:
        return plan
    if G > 8:
        return base._error(E_INVALID, M_MANY)
    if not beauty:
        return base._error(E_INVALID, M_BEAUTY)
    if integrator == VOLUME:
        return base._error(E_UNSUPPORTED, M_VOLUME)
    if adaptive:
        return base._error(E_UNSUPPORTED, M_ADAPTIVE)
    if K or matte or bits or gbits or moment:
        return base._error(E_UNSUPPORTED, M_ALONE)
    plan["outputs"] += [(LIGHT_GROUP, g) for g in range(G)]
    plan["extra"] = 16 * G
    return plan


# the guides' grid: every earlier case, without a guide and with each guide request
GRID = [c + (gbits, 8) for c in base.CASES for gbits in (0, 1, 3)]


def test_new_kind_comes_last_and_has_no_pass(exe):
    out = subprocess.run([exe, "constants"], capture_output=True, text=True, check=True).stdout.split()
    guide_normal, light_group, its_pass, n_passes, max_outputs, n_pass_of, max_groups = map(int, out)
    assert light_group == guide_normal + 1 == guides.GUIDE_NORMAL + 1 == LIGHT_GROUP
    assert its_pass == n_passes == guides.GUIDE_PASS + 1  # the path kernel's own records: no PassKind added
    assert n_pass_of == 8 and max_groups == 8 and max_outputs >= 1 + max_groups


def test_without_groups_the_plan_is_the_earlier_one(checker, tmp_path):
    """G = 0 over the guides' whole grid: the earlier restatement for a frame, and under both rule sets
    the answers of the earlier checker (tests/native/frame_plan_guides_check.cpp), which knows no groups."""
    earlier = str(tmp_path / "frame_plan_guides_check")
    subprocess.check_call([shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-o", earlier,
                           os.path.join(HERE, "native", "frame_plan_guides_check.cpp")])
    for rules in ("frame", "buckets"):
        got = checker([c + (0,) for c in GRID], rules)
        lines = [rules + " %d %d %d %d %d %d %d %d %d %d" % c for c in GRID]
        out = subprocess.run([earlier], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        assert got == [base._parse(a) for a in out.stdout.splitlines()]
        if rules == "frame":
            for c, g in zip(GRID, got):
                assert g == guides.restate(*c), c


def test_groups_match_the_rules(checker):
    cases = [c + (G,) for c in GRID for G in (1, 2, 8, 9)]
    seen = set()
    for c, got in zip(cases, checker(cases)):
        want = restate(*c)
        assert got == want, (c, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
        if got["code"] == 0:
            G = c[-1]
            assert got["outputs"] == [(base.BEAUTY, 0)] + [(LIGHT_GROUP, g) for g in range(G)]  # beauty, then the groups
            assert got["passes"] == [] and got["path"] == 1 and got["extra"] == 16 * G
        seen.add(got["message"])
    for m in (M_MANY, M_BEAUTY, M_VOLUME, M_ADAPTIVE, M_ALONE, ""):
        assert m in seen, m


def test_each_new_rule_alone(checker):
    many, nobeauty, volume, adaptive, cascade, mattes, aovs, gd, moment, ok = checker([
        (1, 0, 0, 0, 0, 0, 0, PATH, 0, 0, 9), (0, 0, 0, 0, 0, 0, 0, PATH, 0, 0, 2), (1, 0, 0, 0, 0, 0, 0, VOLUME, 0, 0, 2),
        (1, 0, 0, 1, 0, 0, 0, PATH, 0, 0, 2), (1, 0, 0, 0, 2, 0, 0, PATH, 0, 0, 2), (1, 0, 0, 0, 0, 1, 4, PATH, 0, 0, 2),
        (1, 1, 0, 0, 0, 0, 0, PATH, 0, 0, 2), (1, 0, 0, 0, 0, 0, 0, PATH, 3, 8, 2), (1, 0, 1, 0, 0, 0, 0, PATH, 0, 0, 2),
        (1, 0, 0, 0, 0, 0, 0, PATH, 0, 0, 8)])
    assert many == base._error(E_INVALID, M_MANY)
    assert nobeauty == base._error(E_INVALID, M_BEAUTY)
    assert volume == base._error(E_UNSUPPORTED, M_VOLUME)
    assert adaptive == base._error(E_UNSUPPORTED, M_ADAPTIVE)
    alone = base._error(E_UNSUPPORTED, M_ALONE)
    assert cascade == alone and mattes == alone and aovs == alone and gd == alone and moment == alone
    assert ok["code"] == 0 and len(ok["outputs"]) == 9 and ok["extra"] == 128


def test_bucket_rules_take_groups_too(checker):
    (got,) = checker([(1, 0, 0, 0, 0, 0, 0, PATH, 0, 0, 3)], rules="buckets")
    assert got["outputs"] == [(base.BEAUTY, 0), (LIGHT_GROUP, 0), (LIGHT_GROUP, 1), (LIGHT_GROUP, 2)] and got["extra"] == 48
