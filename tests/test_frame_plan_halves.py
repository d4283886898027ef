"""The half buffers in the frame plan (csrc/host/frame_plan.h plan_frame), checked on the CPU: two new
output kinds delivered after the followed guides and one new pass, which takes the value after N_PASSES
(pass_of's "no pass", which keeps its value) and still runs first among a frame's passes; the new rules
refuse with their own code and message after every earlier rule; a request without the halves gets
exactly the plan it got before (the cost checker's answers over its whole grid, under both rule sets);
and an accepted halves frame holds 16 bytes of record memory per sample, with both guides too."""
import os
import shutil
import subprocess

import pytest

import test_frame_plan as base
import test_frame_plan_cost as cost
import test_frame_plan_guides as guides

HERE = os.path.dirname(os.path.abspath(__file__))
E_INVALID, E_UNSUPPORTED = base.E_INVALID, base.E_UNSUPPORTED
PATH, VOLUME = base.PATH, base.VOLUME
HALF_A, HALF_B = 10, 11
HALVES_PASS = 6
M_BEAUTY = "the half buffers need the path kernel (the beauty)"
M_ADAPTIVE = "the half buffers need a uniform render: not adaptive sampling"
M_ALONE = ("the half buffers are not rendered with the moment image, the cascade, the mattes, light groups, depth cuts or "
           "the cost image in one call")


def _build(tmp, name):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found")
    path = str(tmp / name)
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-o", path, os.path.join(HERE, "native", name + ".cpp")])
    return path


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("frame_plan_halves"), "frame_plan_halves_check")


@pytest.fixture(scope="module")
def earlier(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("frame_plan_halves_earlier"), "frame_plan_cost_check")


_ask = cost._ask


def restate(beauty, bits, moment, adaptive, K, matte, n_ids, integrator, gbits, max_follow, G, cuts, cost_on, halves):
    """A whole frame's plan with the half buffers: the earlier rules first, then the halves' own in their
    order, each with its message; else the earlier plan with the two halves after its outputs, their
    pass before its passes, and 16 bytes per sample."""
    plan = cost.restate(beauty, bits, moment, adaptive, K, matte, n_ids, integrator, gbits, max_follow, G, cuts, cost_on)
    if plan["code"] or not halves:
        return plan
    if not beauty:
        return base._error(E_INVALID, M_BEAUTY)
    if adaptive:
        return base._error(E_UNSUPPORTED, M_ADAPTIVE)
    if moment or K or matte or G or cuts or cost_on:
        return base._error(E_UNSUPPORTED, M_ALONE)
    plan["outputs"] = plan["outputs"] + [(HALF_A, 0), (HALF_B, 0)]
    plan["passes"] = [HALVES_PASS] + plan["passes"]
    plan["extra"] = 16
    return plan


# the cost image's grid, without the cost image and with it
GRID = [c + (n,) for c in cost.GRID for n in (0, 1)]


def test_new_kinds_come_last_and_the_pass_takes_the_next_value(exe):
    out = subprocess.run([exe, "constants"], capture_output=True, text=True, check=True).stdout.split()
    depth_cut, half_a, half_b, guide_pass, n_passes, halves_pass, slots, pass_a, pass_b, max_outputs, n_pass_of = map(int, out)
    assert (half_a, half_b) == (depth_cut + 1, depth_cut + 2) == (HALF_A, HALF_B)
    # every earlier enumerator keeps its value, N_PASSES (the "no pass" of pass_of) among them
    assert guide_pass == guides.GUIDE_PASS and n_passes == guide_pass + 1 and n_pass_of == 8
    assert halves_pass == n_passes + 1 == HALVES_PASS and slots == halves_pass + 1
    assert pass_a == pass_b == halves_pass
    assert max_outputs >= 5  # the beauty, two AOVs or guides, two halves


def test_without_halves_the_plan_is_the_earlier_one(exe, earlier):
    for rules in ("frame", "buckets"):
        got = _ask(exe, [c + (0,) for c in GRID], rules)
        assert got == _ask(earlier, GRID, rules)
        if rules == "frame":
            for c, g in zip(GRID, got):
                assert g == cost.restate(*c), c


def test_halves_match_the_rules(exe):
    cases = [c + (1,) for c in GRID]
    seen = set()
    accepted = 0
    for c, got in zip(cases, _ask(exe, cases, "frame")):
        want = restate(*c)
        assert got == want, (c, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
        if got["code"] == 0:
            accepted += 1
            assert got["outputs"][0] == (base.BEAUTY, 0) and got["outputs"][-2:] == [(HALF_A, 0), (HALF_B, 0)]
            assert got["passes"][0] == HALVES_PASS and got["passes"][1:] == sorted(got["passes"][1:])
            assert got["path"] == 1 and got["extra"] == 16
        seen.add(got["message"])
    assert accepted
    for m in (M_BEAUTY, M_ADAPTIVE, M_ALONE, ""):
        assert m in seen, m


def test_each_new_rule_alone(exe):
    # beauty bits moment adaptive K matte n_ids integrator gbits max_follow G cuts cost halves
    (nobeauty, adaptive, moment, cascade, mattes, groups, cuts, cost_on, ok, aovs, gd, one_guide, volume, vol_aovs,
     vol_guides) = _ask(exe, [
        (0, 0, 0, 0, 0, 0, 0, PATH, 0, 0, 0, 0, 0, 1), (1, 0, 0, 1, 0, 0, 0, PATH, 0, 0, 0, 0, 0, 1),
        (1, 0, 1, 0, 0, 0, 0, PATH, 0, 0, 0, 0, 0, 1), (1, 0, 0, 0, 2, 0, 0, PATH, 0, 0, 0, 0, 0, 1),
        (1, 0, 0, 0, 0, 1, 4, PATH, 0, 0, 0, 0, 0, 1), (1, 0, 0, 0, 0, 0, 0, PATH, 0, 0, 2, 0, 0, 1),
        (1, 0, 0, 0, 0, 0, 0, PATH, 0, 0, 0, 2, 0, 1), (1, 0, 0, 0, 0, 0, 0, PATH, 0, 0, 0, 0, 1, 1),
        (1, 0, 0, 0, 0, 0, 0, PATH, 0, 0, 0, 0, 0, 1), (1, 3, 0, 0, 0, 0, 0, PATH, 0, 0, 0, 0, 0, 1),
        (1, 0, 0, 0, 0, 0, 0, PATH, 3, 8, 0, 0, 0, 1), (1, 0, 0, 0, 0, 0, 0, PATH, 2, 8, 0, 0, 0, 1),
        (1, 0, 0, 0, 0, 0, 0, VOLUME, 0, 0, 0, 0, 0, 1), (1, 1, 0, 0, 0, 0, 0, VOLUME, 0, 0, 0, 0, 0, 1),
        (1, 0, 0, 0, 0, 0, 0, VOLUME, 1, 8, 0, 0, 0, 1)], "frame")
    assert nobeauty == base._error(E_INVALID, M_BEAUTY)
    assert adaptive == base._error(E_UNSUPPORTED, M_ADAPTIVE)
    alone = base._error(E_UNSUPPORTED, M_ALONE)
    assert moment == alone and cascade == alone and mattes == alone and groups == alone and cuts == alone and cost_on == alone
    halves = [(HALF_A, 0), (HALF_B, 0)]
    assert ok == dict(code=0, message="", outputs=[(base.BEAUTY, 0)] + halves, passes=[HALVES_PASS], path=1, extra=16)
    assert aovs["outputs"] == [(base.BEAUTY, 0), (base.ALBEDO, 0), (base.NORMAL, 0)] + halves
    assert aovs["passes"] == [HALVES_PASS, base.FIRST_HIT_PASS] and aovs["extra"] == 16
    # both guides: the normal records take the halves' buffer once the halves' pass has run -- still 16 bytes
    assert gd["outputs"][0] == (base.BEAUTY, 0) and gd["outputs"][-2:] == halves and len(gd["outputs"]) == 5
    assert gd["passes"] == [HALVES_PASS, guides.GUIDE_PASS] and gd["extra"] == 16
    assert len(one_guide["outputs"]) == 4 and one_guide["passes"] == [HALVES_PASS, guides.GUIDE_PASS] and one_guide["extra"] == 16
    # the volume integrator: the halves need no surfaces, AOVs and guides do
    assert volume == ok
    assert vol_aovs == base._error(E_UNSUPPORTED, "first-hit AOVs need surfaces: the volume integrator has none")
    assert vol_guides == base._error(E_UNSUPPORTED, "followed guides need surfaces: the volume integrator has none")


def test_bucket_rules_take_halves_too(exe):
    (got,) = _ask(exe, [(1, 0, 0, 0, 0, 0, 0, PATH, 0, 0, 0, 0, 0, 1)], "buckets")
    assert got["outputs"] == [(base.BEAUTY, 0), (HALF_A, 0), (HALF_B, 0)] and got["passes"] == [HALVES_PASS] and got["extra"] == 16
