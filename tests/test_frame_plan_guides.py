"""The followed guides in the frame plan (csrc/host/frame_plan.h plan_frame), checked on the CPU:
the new output kinds and the new pass come last in their lists, the new rules refuse with their own
code and message after every earlier rule, a request without a guide gets exactly the plan it got
before (tests/test_frame_plan.py's restatement over its whole case list), and a request with guides
gets that plan plus the guide outputs, the guide pass and the second record buffer."""
import itertools
import os
import shutil
import subprocess

import pytest

import test_frame_plan as base

HERE = os.path.dirname(os.path.abspath(__file__))
E_INVALID, E_UNSUPPORTED = base.E_INVALID, base.E_UNSUPPORTED
PATH, VOLUME = base.PATH, base.VOLUME
GUIDE_ALBEDO, GUIDE_NORMAL = 6, 7
GUIDE_PASS = 4


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found")
    path = str(tmp_path_factory.mktemp("frame_plan_guides") / "frame_plan_guides_check")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-o", path,
                           os.path.join(HERE, "native", "frame_plan_guides_check.cpp")])
    return path


@pytest.fixture(scope="module")
def checker(exe):
    def ask(cases, rules="frame"):
        lines = [rules + " %d %d %d %d %d %d %d %d %d %d" % c for c in cases]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        answers = out.stdout.splitlines()
        assert len(answers) == len(lines)
        return [base._parse(a) for a in answers]
    return ask


def restate(beauty, bits, moment, adaptive, K, matte, n_ids, integrator, gbits, max_follow):
    """A whole frame's plan with followed guides (gbits: 1 albedo, 2 normal): the earlier rules first,
    then the guides' own, each with its message; else the earlier plan plus the guide outputs after
    every other output, the guide pass after every other pass, and 16 bytes of record memory per
    sample where both guides are asked for."""
    plan = base.restate(beauty, bits, moment, adaptive, K, matte, n_ids, integrator)
    if plan["code"] or not gbits:
        return plan
    if integrator == VOLUME:
        return base._error(E_UNSUPPORTED, "followed guides need surfaces: the volume integrator has none")
    if adaptive or K or matte:
        return base._error(E_UNSUPPORTED, "followed guides need a uniform render without the cascade and the mattes")
    if bits:
        return base._error(E_UNSUPPORTED, "followed guides and first-hit AOVs are not rendered in one call")
    if max_follow > 10:
        return base._error(E_INVALID, "max_follow must be 0..10")
    plan["outputs"] += [(kind, 0) for kind, on in ((GUIDE_ALBEDO, gbits & 1), (GUIDE_NORMAL, gbits & 2)) if on]
    plan["passes"].append(GUIDE_PASS)
    plan["extra"] = 16 if gbits == 3 else 0
    return plan


def test_new_kinds_and_pass_come_last(exe):
    out = subprocess.run([exe, "constants"], capture_output=True, text=True, check=True).stdout.split()
    guide_albedo, guide_normal, guide_pass, matte_pass, n_passes, max_outputs, n_pass_of, max_follow = map(int, out)
    assert (guide_albedo, guide_normal) == (base.PLANE + 1, base.PLANE + 2) == (GUIDE_ALBEDO, GUIDE_NORMAL)
    assert guide_pass == matte_pass + 1 == base.MATTE_PASS + 1 == GUIDE_PASS and n_passes == guide_pass + 1
    assert n_pass_of == guide_normal + 1  # one pass per kind
    assert max_outputs >= 4 + 8 + 2 and max_follow == 10


def test_without_guides_the_plan_is_the_earlier_one(checker):
    """Every case of tests/test_frame_plan.py, under both rule sets' entry, with no guide asked for
    (max_follow set or not): the earlier restatement, the earlier checker's answers."""
    for mf in (0, 8, 11):
        cases = [c + (0, mf) for c in base.CASES]
        for c, got in zip(base.CASES, checker(cases)):
            assert got == base.restate(*c), (c, mf)


def test_guides_match_the_rules(checker):
    cases = [c + (gbits, mf) for c in base.CASES for gbits in (1, 2, 3) for mf in ((8,) if c[1] or c[3] else (0, 8, 10, 11))]
    seen = set()
    for c, got in zip(cases, checker(cases)):
        want = restate(*c)
        assert got == want, (c, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
        if got["code"] == 0:
            assert got["path"] == c[0] and got["passes"][-1] == GUIDE_PASS
            assert got["outputs"] == sorted(got["outputs"]) and len(got["outputs"]) <= 4  # beauty, moment, two guides
        seen.add((got["code"], got["message"]))
    messages = {m for _c, m in seen}
    for m in ("followed guides need surfaces: the volume integrator has none",
              "followed guides need a uniform render without the cascade and the mattes",
              "followed guides and first-hit AOVs are not rendered in one call", "max_follow must be 0..10", ""):
        assert m in messages, m


def test_each_new_rule_alone(checker):
    volume, adaptive, cascade, mattes, aovs, deep = checker([
        (1, 0, 0, 0, 0, 0, 0, VOLUME, 3, 8), (1, 0, 0, 1, 0, 0, 0, PATH, 3, 8), (1, 0, 0, 0, 2, 0, 0, PATH, 1, 8),
        (1, 0, 0, 0, 0, 1, 4, PATH, 2, 8), (1, 1, 0, 0, 0, 0, 0, PATH, 3, 8), (1, 0, 0, 0, 0, 0, 0, PATH, 3, 11)])
    assert volume == base._error(E_UNSUPPORTED, "followed guides need surfaces: the volume integrator has none")
    uniform = base._error(E_UNSUPPORTED, "followed guides need a uniform render without the cascade and the mattes")
    assert adaptive == uniform and cascade == uniform and mattes == uniform
    assert aovs == base._error(E_UNSUPPORTED, "followed guides and first-hit AOVs are not rendered in one call")
    assert deep == base._error(E_INVALID, "max_follow must be 0..10")


def test_spot_checks(checker):
    both, one, alone, moment, buckets = checker([
        (1, 0, 0, 0, 0, 0, 0, PATH, 3, 8), (1, 0, 0, 0, 0, 0, 0, PATH, 2, 0), (0, 0, 0, 0, 0, 0, 0, PATH, 3, 10),
        (1, 0, 1, 0, 0, 0, 0, PATH, 3, 8)]) + checker([(1, 0, 0, 0, 0, 0, 0, PATH, 1, 3)], rules="buckets")
    assert both["outputs"] == [(base.BEAUTY, 0), (GUIDE_ALBEDO, 0), (GUIDE_NORMAL, 0)]
    assert both["passes"] == [GUIDE_PASS] and both["extra"] == 16 and both["path"] == 1
    assert one["outputs"] == [(base.BEAUTY, 0), (GUIDE_NORMAL, 0)] and one["extra"] == 0  # one record: no extra memory
    assert alone["path"] == 0 and alone["outputs"] == [(GUIDE_ALBEDO, 0), (GUIDE_NORMAL, 0)]  # no path kernel
    assert moment["outputs"] == [(base.BEAUTY, 0), (base.MOMENT, 0), (GUIDE_ALBEDO, 0), (GUIDE_NORMAL, 0)]
    assert moment["passes"] == [base.MOMENT_PASS, GUIDE_PASS]  # the guides overwrite d_L: after the moment pass
    assert buckets["outputs"] == [(base.BEAUTY, 0), (GUIDE_ALBEDO, 0)] and buckets["passes"] == [GUIDE_PASS]
