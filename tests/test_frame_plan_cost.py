"""The cost image in the frame plan (csrc/host/frame_plan.h plan_frame), checked on the CPU: the cost grid
is not a tile image, so a cost frame adds no output kind and no pass; the new rules refuse with their own
code and message after every earlier rule; a request without the cost image gets exactly the plan it got
before (the depth-cut checker's answers over its whole grid, under both rule sets); and an accepted cost
frame is the beauty alone with 16 bytes of record memory per sample."""
import os
import shutil
import subprocess

import pytest

import test_frame_plan as base
import test_frame_plan_depth as depth

HERE = os.path.dirname(os.path.abspath(__file__))
E_INVALID, E_UNSUPPORTED = base.E_INVALID, base.E_UNSUPPORTED
PATH, VOLUME = base.PATH, base.VOLUME
M_BEAUTY = "the cost image needs the path kernel (the beauty)"
M_VOLUME = "the cost image needs the path integrator: the volume integrator has no cost build"
M_ADAPTIVE = "the cost image needs a uniform render: not adaptive sampling"
M_ALONE = ("the cost image is not rendered with the cascade, the mattes, AOVs, guides, the moment image, light groups or "
           "depth cuts in one call")


def _build(tmp, name):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found")
    path = str(tmp / name)
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-o", path, os.path.join(HERE, "native", name + ".cpp")])
    return path


def _ask(exe, cases, rules):
    lines = [rules + " " + " ".join("%d" % v for v in c) for c in cases]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    answers = out.stdout.splitlines()
    assert len(answers) == len(lines)
    return [base._parse(a) for a in answers]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("frame_plan_cost"), "frame_plan_cost_check")


@pytest.fixture(scope="module")
def earlier(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("frame_plan_cost_earlier"), "frame_plan_depth_check")


def restate(beauty, bits, moment, adaptive, K, matte, n_ids, integrator, gbits, max_follow, G, cuts, cost):
    """A whole frame's plan with the cost image: the earlier rules first, then the cost image's own in
    their order, each with its message; else the beauty alone, no pass, 16 bytes per sample."""
    plan = depth.restate(beauty, bits, moment, adaptive, K, matte, n_ids, integrator, gbits, max_follow, G, cuts)
    if plan["code"] or not cost:
        return plan
    if not beauty:
        return base._error(E_INVALID, M_BEAUTY)
    if integrator == VOLUME:
        return base._error(E_UNSUPPORTED, M_VOLUME)
    if adaptive:
        return base._error(E_UNSUPPORTED, M_ADAPTIVE)
    if K or matte or bits or gbits or moment or G or cuts:
        return base._error(E_UNSUPPORTED, M_ALONE)
    plan["extra"] = 16
    return plan


# the depth cuts' grid, without cuts and with two
GRID = [c + (n,) for c in depth.GRID for n in (0, 2)]


def test_no_new_kind_and_no_new_pass(exe, earlier):
    last_kind, n_passes, max_outputs, n_pass_of = map(int, subprocess.run([exe, "constants"], capture_output=True, text=True,
                                                                       check=True).stdout.split())
    before = list(map(int, subprocess.run([earlier, "constants"], capture_output=True, text=True, check=True).stdout.split()))
    assert last_kind == depth.DEPTH_CUT == before[1]
    assert n_pass_of == 8 and n_passes == before[3] and max_outputs == before[4]


def test_without_cost_the_plan_is_the_earlier_one(exe, earlier):
    for rules in ("frame", "buckets"):
        got = _ask(exe, [c + (0,) for c in GRID], rules)
        assert got == _ask(earlier, GRID, rules)
        if rules == "frame":
            for c, g in zip(GRID, got):
                assert g == depth.restate(*c), c


def test_cost_matches_the_rules(exe):
    cases = [c + (1,) for c in GRID]
    seen = set()
    for c, got in zip(cases, _ask(exe, cases, "frame")):
        want = restate(*c)
        assert got == want, (c, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
        if got["code"] == 0:
            assert got["outputs"] == [(base.BEAUTY, 0)]  # the beauty alone: the grid is no tile image
            assert got["passes"] == [] and got["path"] == 1 and got["extra"] == 16
        seen.add(got["message"])
    for m in (M_BEAUTY, M_VOLUME, M_ADAPTIVE, M_ALONE, ""):
        assert m in seen, m


def test_each_new_rule_alone(exe):
    nobeauty, volume, adaptive, cascade, mattes, aovs, gd, moment, groups, cuts, ok = _ask(exe, [
        (0, 0, 0, 0, 0, 0, 0, PATH, 0, 0, 0, 0, 1), (1, 0, 0, 0, 0, 0, 0, VOLUME, 0, 0, 0, 0, 1),
        (1, 0, 0, 1, 0, 0, 0, PATH, 0, 0, 0, 0, 1), (1, 0, 0, 0, 2, 0, 0, PATH, 0, 0, 0, 0, 1),
        (1, 0, 0, 0, 0, 1, 4, PATH, 0, 0, 0, 0, 1), (1, 1, 0, 0, 0, 0, 0, PATH, 0, 0, 0, 0, 1),
        (1, 0, 0, 0, 0, 0, 0, PATH, 3, 8, 0, 0, 1), (1, 0, 1, 0, 0, 0, 0, PATH, 0, 0, 0, 0, 1),
        (1, 0, 0, 0, 0, 0, 0, PATH, 0, 0, 2, 0, 1), (1, 0, 0, 0, 0, 0, 0, PATH, 0, 0, 0, 2, 1),
        (1, 0, 0, 0, 0, 0, 0, PATH, 0, 0, 0, 0, 1)], "frame")
    assert nobeauty == base._error(E_INVALID, M_BEAUTY)
    assert volume == base._error(E_UNSUPPORTED, M_VOLUME)
    assert adaptive == base._error(E_UNSUPPORTED, M_ADAPTIVE)
    alone = base._error(E_UNSUPPORTED, M_ALONE)
    assert cascade == alone and mattes == alone and aovs == alone and gd == alone and moment == alone
    assert groups == alone and cuts == alone
    assert ok["code"] == 0 and ok["outputs"] == [(base.BEAUTY, 0)] and ok["passes"] == [] and ok["extra"] == 16
