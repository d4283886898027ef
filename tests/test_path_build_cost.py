"""The cost build in plan_build (csrc/host/path_build.h), checked on the CPU over the grid of
tests/test_path_build.py: with cost the answer is always the generic two-wave build without priority
lanes, {fm = FT_ALL, wv = 2, pr = false, count = false, cs = true}, ext and env as before, for every
specialize setting and with the counter pass on or off -- never a lean or specialised build, never the
counter, light-group or depth-cut build -- and plan_path then gives no priority or pair schedule and
launches no k_primary; where plan_build would run k_render (variant 3, or a BVH deeper than the ray-queue
LDS holds) it refuses, naming the cost image; without cost the answers are the earlier ones."""
import os
import shutil
import subprocess

import pytest

import test_path_build as base
from nart_amd.api import FT_ALL, SCHED

HERE = os.path.dirname(os.path.abspath(__file__))
REFUSAL = "the cost image needs the ray-queue kernel: not variant 3, nor a BVH deeper than its LDS holds"
# the instantiations render.hip's table adds: {ext, count, env, fm, wv, pr, lg, dc, cs}
CS_BUILDS = {(e, 0, v, FT_ALL, 2, 0, 0, 0, 1) for e in (0, 1) for v in (0, 1)}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found")
    d = tmp_path_factory.mktemp("path_build_cost")
    exes = {}
    for name in ("path_build_cost_check", "path_build_depth_check"):
        exes[name] = str(d / name)
        subprocess.check_call([hipcc, "-O2", "-std=c++17", "-o", exes[name], os.path.join(HERE, "native", name + ".cpp")])

    def ask(lines, earlier=False):
        out = subprocess.run([exes["path_build_depth_check" if earlier else "path_build_cost_check"]],
                             input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        answers = out.stdout.splitlines()
        assert len(answers) == len(lines)
        return answers
    return ask


def _split(line):
    text, message = line.split(" # ") if not line.endswith(" # ") else (line[:-3], "")
    got = base._fields(text)
    plan = {k[2:]: got.pop(k) for k in list(got) if k.startswith("p_")}
    return got, plan, message


def test_cost_always_takes_the_generic_two_wave_build(checker):
    cases = list(base._build_cases())
    seen, refused, specs, counter_cases = set(), 0, set(), set()
    for (c, kn), line in zip(cases, checker([base._build_line(c, kn) + " 0 1" for c, kn in cases])):
        got, plan, message = _split(line)
        features, env, spec, counters, bounces, variant, depth = c[:7]
        want_rq = base.restate_build(*c, kn=kn)["rq"]
        build = tuple(got[k] for k in ("ext", "count", "env", "fm", "wv", "pr", "lg", "dc", "cs"))
        assert build == (int(bounces > 10), 0, env, FT_ALL, 2, 0, 0, 0, 1), (c, kn, build)
        assert build in CS_BUILDS and got["rq"] == want_rq and got["rq_block"] == 512 and got["stack_lds"] == depth
        specs.add(spec)
        counter_cases.add(counters)
        if not want_rq:  # k_render would run: refused, as a combination that has no kernel
            assert got["error"] == 1 and got["unsupported"] == 1 and message == REFUSAL, (c, kn)
            assert "cost image" in message
            assert variant == 3 or base.rq_fixed_lds(depth, 512) > int(min(base._num(kn, "NART_RQ_LDS_LIMIT", base.CU_LDS), base.CU_LDS))
            refused += 1
            continue
        assert got["error"] == 0 and got["unsupported"] == 0 and message == "" and got["fm_used"] == FT_ALL
        assert got["rq_lds"] <= base.CU_LDS
        # plan_path: no priority lanes, no speculative pairs, no half waves, no lean or specialised bit, no k_primary
        names = {k for k, bit in SCHED.items() if plan["sched"] & bit}
        assert not names & {"priority", "spec_pairs", "half_waves", "lean", "specialized", "primary"}, (c, names)
        assert not (plan["rq_prio"] or plan["pairs"] or plan["half"] or plan["quad"]) and not plan["error"]
        seen.add((build, plan["shape"]))
    assert {s[0] for s in seen} == CS_BUILDS and refused
    assert specs == {0, 1, 2} and counter_cases == {0, 1}  # every specialize setting, counter pass on and off
    assert {s[1] for s in seen} >= {base.DIRECT, base.GROUPS, base.PIXEL_QUEUE}  # small shards run the plain schedule


def test_without_cost_the_answers_are_the_earlier_ones(checker):
    cases = list(base._build_cases())
    lines = [base._build_line(c, kn) for c, kn in cases]
    for dc in (0, 1):
        now, before = checker([l + " %d 0" % dc for l in lines]), checker([l + " %d" % dc for l in lines], earlier=True)
        for (c, kn), a, b in zip(cases, now, before):
            got, plan, message = _split(a)
            assert got.pop("cs") == 0
            assert (got, plan, message) == _split(b), (c, kn)
