"""The depth-cut build in plan_build (csrc/host/path_build.h), checked on the CPU over the grid of
tests/test_path_build.py: with depth_cuts the answer is always the generic two-wave build without
priority lanes, {fm = FT_ALL, wv = 2, pr = false, dc = true}, ext and env as before -- never a lean or
specialised build, never the counter or the light-group build -- and plan_path then gives no priority or
pair schedule; where plan_build would run k_render (variant 3, or a BVH deeper than the ray-queue LDS
holds) it refuses, naming depth cuts; without depth_cuts the answers are the earlier ones."""
import os
import shutil
import subprocess

import pytest

import test_path_build as base
from nart_amd.api import FT_ALL, SCHED

HERE = os.path.dirname(os.path.abspath(__file__))
REFUSAL = "depth cuts need the ray-queue kernel: not variant 3, nor a BVH deeper than its LDS holds"
# the instantiations render.hip's table adds: {ext, count, env, fm, wv, pr, lg, dc}
DC_BUILDS = {(e, 0, v, FT_ALL, 2, 0, 0, 1) for e in (0, 1) for v in (0, 1)}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found")
    d = tmp_path_factory.mktemp("path_build_depth")
    exes = {}
    for name in ("path_build_depth_check", "path_build_check"):
        exes[name] = str(d / name)
        subprocess.check_call([hipcc, "-O2", "-std=c++17", "-o", exes[name], os.path.join(HERE, "native", name + ".cpp")])

    def ask(lines, earlier=False):
        out = subprocess.run([exes["path_build_check" if earlier else "path_build_depth_check"]],
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


def test_depth_cuts_always_take_the_generic_two_wave_build(checker):
    cases = list(base._build_cases())
    seen, refused = set(), 0
    for (c, kn), line in zip(cases, checker([base._build_line(c, kn) + " 1" for c, kn in cases])):
        got, plan, message = _split(line)
        features, env, spec, counters, bounces, variant, depth = c[:7]
        want_rq = base.restate_build(*c, kn=kn)["rq"]
        build = tuple(got[k] for k in ("ext", "count", "env", "fm", "wv", "pr", "lg", "dc"))
        assert build == (int(bounces > 10), 0, env, FT_ALL, 2, 0, 0, 1), (c, kn, build)
        assert build in DC_BUILDS and got["rq"] == want_rq and got["rq_block"] == 512 and got["stack_lds"] == depth
        if not want_rq:  # k_render would run: refused, as a combination that has no kernel
            assert got["error"] == 1 and got["unsupported"] == 1 and message == REFUSAL, (c, kn)
            assert "depth cuts" in message
            assert variant == 3 or base.rq_fixed_lds(depth, 512) > int(min(base._num(kn, "NART_RQ_LDS_LIMIT", base.CU_LDS), base.CU_LDS))
            refused += 1
            continue
        assert got["error"] == 0 and got["unsupported"] == 0 and message == "" and got["fm_used"] == FT_ALL
        assert got["rq_lds"] <= base.CU_LDS
        # plan_path: no priority lanes, no speculative pairs, no half waves, no lean or specialised bit
        names = {k for k, bit in SCHED.items() if plan["sched"] & bit}
        assert not names & {"priority", "spec_pairs", "half_waves", "lean", "specialized"}, (c, names)
        assert not (plan["rq_prio"] or plan["pairs"] or plan["half"] or plan["quad"]) and not plan["error"]
        seen.add((build, plan["shape"]))
    assert {s[0] for s in seen} == DC_BUILDS and refused
    assert {s[1] for s in seen} >= {base.DIRECT, base.GROUPS, base.PIXEL_QUEUE}  # small shards run the plain schedule


def test_without_depth_cuts_the_answers_are_the_earlier_ones(checker):
    cases = list(base._build_cases())
    lines = [base._build_line(c, kn) for c, kn in cases]
    now, before = checker([l + " 0" for l in lines]), checker(lines, earlier=True)
    for (c, kn), a, b in zip(cases, now, before):
        got, plan, message = _split(a)
        assert got.pop("lg") == 0 and got.pop("dc") == 0 and got.pop("unsupported") == 0
        assert (got, plan, message) == _split(b), (c, kn)
